"""ddp_stage_a_gh3's store-wave kernel (ddp_stage_a_g3dw_kernel: 3 MFMA waves + 1 store wave per workgroup) against the four symmetric
waves it replaces for long products: the two write the SAME BYTES - G planes, Gb, padding - and raise range_flag alike, whatever tile or
workgroup a row sits in.  ddp_sa_drainwave (include/ddp_hip.h) selects the form: 0 = symmetric, 2 = store wave for every product.
The symmetric form is only the yardstick HERE: tests/test_gpu_stage_a_planes_fp64.py is where both forms meet the definition (fp64, byte for byte)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

K, LDX = 60, 184          # hid = 180: the three 60-wide inputs of a node row, at offsets 0 / 60 / 120
L3 = 13440                # the layer-3 product: gh3_ld(180, 72) / 6 * 8 columns


def _dest(ncols, nplane):
    """gh_dest of plane form 1 (packing.gh_dest_table): group g at float 6 g of the row; bit 0 = a plane group (the first `nplane`)."""
    g = torch.arange(ncols // 8, dtype=torch.int64)
    tab = torch.stack([6 * g, 6 * g + 4], dim=1).int()
    tab[:nplane, 0] += 1
    return tab


class _Form:
    def __init__(self, lib, mode):
        self.var, self.mode = C.c_int.in_dll(lib, "ddp_sa_drainwave"), mode

    def __enter__(self):
        self.old = self.var.value
        self.var.value = self.mode

    def __exit__(self, *a):
        self.var.value = self.old


def _both(nrows, ncols, nb=1, nplanes=None, rows=None, out_rows=None, nrows_dev=None, spike=None, new_mode=2, seed=0, k=K, ldx=LDX, off=60):
    """The raw output words and the flag of both forms on one seeded product."""
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import packing as P
    from diffdock_pocket_amd.launch import stream
    lib = L.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    n_x = out_rows if rows is not None else nrows
    x = torch.randn(n_x, ldx, generator=g)
    if spike is not None:
        x[spike[0], spike[1]] = spike[2]
    W = torch.randn(nb, k, ncols, generator=g) * 0.3
    xd, Wd = x.to(dev), W.to(dev)
    wh = P.split_h2(Wd, unified_scale=P.GH_SW)
    nplanes = nplanes or [ncols // 8 - 3] * nb
    dest = torch.stack([_dest(ncols, p) for p in nplanes]).contiguous().to(dev)
    ld = ncols // 8 * 6
    offs = (C.c_int32 * nb)(*[off * (i % 3) for i in range(nb)])
    rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=dev)
    cnt_d = None if nrows_dev is None else torch.tensor([nrows_dev], dtype=torch.int32, device=dev)
    res = []
    for mode in (0, new_mode):
        out = torch.full((nb, n_x, ld), float("nan"), device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        with _Form(lib, mode):
            L.check(lib.ddp_stage_a_gh3(xd.data_ptr(), ldx, nrows, None if rows_d is None else rows_d.data_ptr(),
                                        None if cnt_d is None else cnt_d.data_ptr(), n_x, offs, nb, Wd.data_ptr(), wh.data_ptr(), k, ncols,
                                        out.data_ptr(), ld, flag.data_ptr(), dest.data_ptr(), stream()), "ddp_stage_a_gh3")
        torch.cuda.synchronize()
        res.append((out.view(torch.int32).cpu(), int(flag.item())))
    return res


def _same(res, flag=0, written=True):
    (a, fa), (b, fb) = res
    assert fa == flag and fb == flag, (fa, fb)
    assert torch.equal(a, b)
    nan = torch.tensor(float("nan")).view(torch.int32)
    assert bool((a != nan).any()) == written


@pytest.mark.parametrize("nrows", [1, 31, 32, 33, 63, 65, 257])
def test_rows_at_tile_and_workgroup_edges(nrows):
    """512 columns: a workgroup with all three row groups and one with a single group; 3 products."""
    _same(_both(nrows, 512, nb=3))


@pytest.mark.parametrize("ncols", [128, 256])
def test_one_and_two_column_groups(ncols):
    _same(_both(65, ncols, nb=1))


@pytest.mark.parametrize("nb", [1, 2])
def test_layer3_width_with_and_without_the_second_slot(nb):
    """The real width (35 full workgroups); the second G slot is a product with a plane-group count of its own."""
    _same(_both(65, L3, nb=nb, nplanes=[23 * 72, 23 * 28][:nb]))


def test_row_list_with_repeats_unsorted():
    g = torch.Generator().manual_seed(3)
    rows = torch.randint(0, 300, (257,), generator=g).tolist()
    rows[10] = rows[200] = rows[0]
    _same(_both(257, 256, nb=3, rows=rows, out_rows=300))


@pytest.mark.parametrize("count", [0, 33, 200])
def test_device_side_length_below_capacity(count):
    rows = torch.randperm(300, generator=torch.Generator().manual_seed(4))[:257].tolist()
    _same(_both(257, 256, nb=1, rows=rows, out_rows=300, nrows_dev=count), written=count > 0)


def test_long_list_walks_its_tiles():
    """More tiles than the bounded grid of a listed product has workgroups: every workgroup walks several row ranges."""
    rows = torch.randperm(12600, generator=torch.Generator().manual_seed(5))[:12500].tolist()
    _same(_both(12500, 128, nb=1, rows=rows, out_rows=12600, nrows_dev=12400))


def test_dense_product_walks_its_row_ranges():
    """A dense product on the store-wave form's bounded grid: at the layer-3 width two products leave 7 ranges of 128 rows a time, so
    2000 rows are 16 ranges (the last of 80 rows: two tiles and a half) walked by 7 workgroups per column group."""
    _same(_both(2000, L3, nb=2, nplanes=[23 * 72, 23 * 28]))


@pytest.mark.parametrize("ldx,off", [(181, 60), (184, 61)])
def test_x_rows_that_are_not_16_byte_aligned(ldx, off):
    """An odd row stride / an odd column offset of x: the loop variant that fetches x with 4-byte loads; dense and listed."""
    _same(_both(65, 512, nb=3, ldx=ldx, off=off))
    rows = torch.randperm(100, generator=torch.Generator().manual_seed(6))[:65].tolist()
    _same(_both(65, 256, nb=2, rows=rows, out_rows=100, ldx=ldx, off=off))


@pytest.mark.parametrize("k", [32, 24, 16])
def test_the_other_inner_sizes(k):
    """K = 32 / 24 / 16 (one or two 16-deep MFMA steps, with and without k padding): their own instantiations of both kernels."""
    _same(_both(97, 512, nb=2, k=k, ldx=64, off=16))


def test_default_dispatch_takes_the_same_bytes():
    """Mode 1 (the default: the store wave from 4096 rows on), a dense product of 384 columns: one full workgroup per row range."""
    _same(_both(4100, 384, nb=2, new_mode=1))


def test_value_beyond_fp16_range_raises_the_flag_in_both_forms():
    _same(_both(65, 256, nb=1, spike=(40, 3, 40000.0)), flag=1)


def test_forward_through_plane_form_1_is_bitwise_equal():
    """cfg2_small (ns = 60, hid = 180: every factorised conv runs ddp_conv_rows on G in plane form 1, so its stage A is ddp_stage_a_gh3)
    forward under both kernels: the scores are equal bit for bit."""
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import launch as K_
    from diffdock_pocket_amd.score_model import TensorProductScoreModel
    from oracle.cases import CASES
    from oracle.weights import synth_state_dict
    lib = L.load()
    dev = torch.device("cuda:0")
    case = CASES["cfg2_small"]
    kw = dict(case.model_kwargs())
    kw.update(case.ctor_extras())
    kw["device"] = dev
    outs = []
    for mode in (0, 2):
        with _Form(lib, mode):
            model = TensorProductScoreModel(**kw)
            model.load_state_dict(synth_state_dict(model.state_dict(), seed=0))
            model = model.to(dev).eval()
            got = model(case.make_batch().to(dev))
            torch.cuda.synchronize()
            # the forward did go through ddp_stage_a_gh3: every factorised conv is on the rows path with G in plane form 1
            paths = [K_.conv_path(c.packed_g(dev), model.rows_all_or_none(dev)) for c in model.conv_layers]
            assert paths and all(p.rows and p.gh_fmt == 1 for p in paths)
            outs.append([t.detach().float().cpu() for t in got])
    assert sum(a.numel() for a in outs[0]) > 0
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.equal(a, b)
