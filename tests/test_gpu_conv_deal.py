"""The tile order of the conv launches (ddp_conv_deal, include/ddp_hip.h; ddp_deal_tile, csrc/ddp_conv_deal.h) decides which workgroup
computes a tile and nothing else: the message arrays of a launch are the SAME BYTES under one contiguous range of tiles per XCD (0) and
under chunks of c tiles dealt to the XCDs in turn - several tasks with unequal edge counts in one launch, host and device-side counts,
tile counts below one super-row of 8 c tiles (the whole launch keeps the range order), one super-row and a remainder, several.

The tasks, their inputs and packs are the ones of test_gpu_conv_messages_fp64.py (which holds them to the float64 definition)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_conv_messages_fp64 as M
from helpers import _bits

pytestmark = pytest.mark.gpu


class _Deal:
    def __init__(self, c):
        from diffdock_pocket_amd import _lib as L
        self.var, self.c = C.c_int.in_dll(L.load(), "ddp_conv_deal"), c

    def __enter__(self):
        self.old = self.var.value
        self.var.value = self.c

    def __exit__(self, *a):
        self.var.value = self.old


def _launch_bits(shape, name, sizes, counts, c):
    """One launch of len(sizes) tasks (own weights, inputs and message buffers) under ddp_conv_deal = c -> the raw words of every msg array
    (guard rows and the rows behind a device-side count included) and the range flag."""
    L, K, P = M._api()
    fact = M.FORMS[name][0]
    flag = torch.zeros(1, dtype=torch.int32, device=M._dev())
    K.set_range_flag(flag)
    try:
        eds, tasks = [], []
        for i, (n, cnt) in enumerate(zip(sizes, counts)):
            conv = M._conv(*shape, seed=i)
            # (a device-side count: the capacity lies 7 above the live edges, the entries behind the count name NaN rows)
            ed = M.Edges(conv, n, 24, seed=300 + i, fact=fact, engine=True, tail=0 if cnt is None else 7)
            if cnt is not None:
                ed.count(cnt)
            ts, spec = M._tasks(conv, name, ed)
            assert all(t.h2_range_flag for t in ts)
            eds.append(ed)
            tasks += ts
        # (stage A of the tasks' G has run over EVERY node row, the all-NaN ones no edge names included, and reported them: the flag is
        # the conv launch's from here on)
        flag.zero_()
        with _Deal(c):
            K.launch_convs(spec, tasks)
        torch.cuda.synchronize()
    finally:
        K.set_range_flag(None)
    return [_bits(ed.msg.cpu().numpy()).copy() for ed in eds], int(flag.item())


# (shape, kernel form, edge tile): the row-stationary kernels of both size classes they have, both MFMA forms; the direct shape; and the
# 32-edge kernel (the form of the size classes without a rows kernel: ns = 16 / nv = 4), which takes its tiles through the same function
LAUNCHES = [((60, 10, 1), "frows_11", 128), ((32, 6, 3), "frows_11", 128), ((60, 10, 1), "frows_00", 128), ((16, 4, 2), "f32_h2", 32)]
# edges per task: 2 + 6 + 1 = 9 tiles of 128 (neither a multiple of 8 nor of 8 c; the last wave of task 0's last tile holds 2 valid
# edges, task 2 has one partial tile) - below 8 c for c >= 2, one super-row and a remainder for c = 1; then 2 + 34 + 1 = 37 tiles: a
# super-row of 32 and a remainder of 5 for c = 4, the range order for c = 8
SIZES = {9: (130, 700, 40), 37: (130, 4300, 40)}


@pytest.mark.parametrize("dev_counts", [False, True], ids=["host_counts", "device_counts"])
@pytest.mark.parametrize("shape,name,T", LAUNCHES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_three_tasks_same_bytes_under_every_order(shape, name, T, dev_counts):
    from diffdock_pocket_amd import _lib as L
    lib = L.load()
    for tiles128, sizes in SIZES.items():
        counts = [n if dev_counts else None for n in sizes]      # (device-side: the count below the capacity n + 7)
        ntl = sum(-(-n // T) for n in sizes)
        assert T != 128 or ntl == tiles128
        want, flag0 = _launch_bits(shape, name, sizes, counts, 0)
        assert flag0 == 0
        assert all(np.isfinite(w.view(np.float32)[:n]).all() for w, n in zip(want, sizes))
        orders = {0: tuple(lib.ddp_conv_deal_tile(i, ntl, 0) for i in range(ntl))}
        for c in (1, 2, 4, 8):
            orders[c] = tuple(lib.ddp_conv_deal_tile(i, ntl, c) for i in range(ntl))
            got, flag = _launch_bits(shape, name, sizes, counts, c)
            assert flag == 0
            for i, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g, w), f"{shape} {name} {sizes} c={c}: task {i} differs from the range order"
        # the launches did run in different orders (c = 1 always deals: 8 <= ntl), and c with 8 c > ntl is the range order itself
        assert orders[1] != orders[0]
        assert all(orders[c] == orders[0] for c in (1, 2, 4, 8) if 8 * c > ntl)
        if ntl >= 32:
            assert orders[4] != orders[0] and orders[4] != orders[1]


def test_direct_shape_same_bytes_under_every_order():
    """One direct-shape task of 200 edges (two tiles: the range order whatever c), then three tasks of segment ranges of 1100 edges: 27
    workgroups, dealt for c = 1 and 2."""
    for name, n in (("drows16", 200), ("drows16x3", 1100)):
        conv = M._conv(60, 10, 1)
        L, K, P = M._api()
        res = {}
        for c in (0, 1, 2, 8):
            flag = torch.zeros(1, dtype=torch.int32, device=M._dev())
            K.set_range_flag(flag)
            try:
                ed = M.Edges(conv, n, 24, seed=77, fact=False, engine=True)
                ts, spec = M._tasks(conv, name, ed)
                assert all(t.h2_range_flag for t in ts)
                with _Deal(c):
                    K.launch_convs(spec, ts)
                torch.cuda.synchronize()
            finally:
                K.set_range_flag(None)
            assert int(flag.item()) == 0
            res[c] = _bits(ed.msg.cpu().numpy()).copy()
        assert np.isfinite(res[0].view(np.float32)[:n]).all()
        for c in (1, 2, 8):
            assert np.array_equal(res[c], res[0]), (name, c)


def test_forward_is_bitwise_equal_under_both_orders():
    """One forward of cfg2_small (every factorised conv through ddp_conv_rows) with the chunks dealt and with one range per XCD."""
    from diffdock_pocket_amd.score_model import TensorProductScoreModel
    from oracle.cases import CASES
    from oracle.weights import synth_state_dict
    dev = torch.device("cuda:0")
    case = CASES["cfg2_small"]
    kw = dict(case.model_kwargs())
    kw.update(case.ctor_extras())
    kw["device"] = dev
    outs = []
    for c in (0, 1, 8):
        with _Deal(c):
            model = TensorProductScoreModel(**kw)
            model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
            model = model.to(dev).eval()
            got = model(case.make_batch().to(dev))
            torch.cuda.synchronize()
            outs.append([t.detach().float().cpu() for t in got])
    assert sum(a.numel() for a in outs[0]) > 0
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert a.shape == b.shape and torch.equal(a, b)
