"""Stage A's plane forms against their DEFINITION at ragged shapes: ddp_stage_a_gh (form 0), ddp_stage_a_gh3 on its four symmetric waves
(ddp_sa_drainwave = 0) and on its store-wave kernel (= 2), and the default dispatch (= 1) where named.  No case uses another kernel's output
as its expected value: the written bytes are either decoded (helpers.decode_gh_rows) and held against an fp64 product inside the bounds of
test_gpu_parity.py::test_stage_a_plane_forms_against_fp64, or - for operands whose accumulator is known exactly - compared word for word with
tests/stage_a_ref64.encode_gh_rows, the numpy statement of include/ddp_hip.h's two forms.

Every launch: `out` starts as a NaN pattern no result can be, x is NaN in every column no product of the launch may fetch and in every row
that is not live, range_flag starts at 0 and is asserted.  A case prints its worst err / bound ("stage_a_fp64 ..." lines, pytest -s):
profiles/stage_a_planes_fp64.txt is that output."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import stage_a_ref64 as R
from helpers import decode_gh_rows

pytestmark = pytest.mark.gpu

FORMS = {"gh": (0, None), "gh3_sym": (1, 0), "gh3_dw": (1, 2), "gh3_default": (1, 1)}      # name -> (plane form, ddp_sa_drainwave)
THREE = ["gh", "gh3_sym", "gh3_dw"]
SENTINEL = np.array([np.nan], dtype=np.float32).view(np.int32)[0]
# the narrowest products: form 1 takes any multiple of 128 columns, form 0 needs the wide path (stage_a_impl: ncols >= 1024)
NCOLS = {0: 1024, 1: 512}
# (n8, part widths) of three products with plane-group counts of their own (60 / 40 / 48): Gb and padding start at different groups
PRODS3 = [(5, [8, 4]), (5, [4, 4]), (4, [12])]


class _Form:
    def __init__(self, lib, mode):
        self.var, self.mode = C.c_int.in_dll(lib, "ddp_sa_drainwave"), mode

    def __enter__(self):
        self.old = self.var.value
        self.var.value = self.mode

    def __exit__(self, *a):
        self.var.value = self.old


class Case:
    """x [n_x, ldx] (NaN wherever no product may read), per product its offset, (n8, widths), plane / Gb weights and right-hand side."""

    def __init__(self, form, n_x, ldx, offs, k, prods, ncols=None, rows=None, count=None):
        self.form, self.fmt = form, FORMS[form][0]
        self.n_x, self.ldx, self.offs, self.k, self.prods = n_x, ldx, list(offs), k, list(prods)
        self.ncols = ncols or NCOLS[self.fmt]
        self.ld = R.row_floats(self.ncols, self.fmt)
        self.rows, self.count = rows, count
        assert len(self.offs) == len(self.prods) and all(0 <= o and o + k <= ldx for o in self.offs)
        if rows is None:
            self.live = np.ones(n_x, dtype=bool)
        else:
            assert all(0 <= r < n_x for r in rows)
            self.live = np.zeros(n_x, dtype=bool)
            self.live[np.asarray(rows[:len(rows) if count is None else count], dtype=np.int64)] = True
        self.fetched = np.zeros(ldx, dtype=bool)
        for o in self.offs:
            self.fetched[o:o + k] = True
        self.x, self.Wv, self.Wb = None, [], []

    def poison(self):
        self.x[:, ~self.fetched] = np.nan
        self.x[~self.live] = np.nan

    def random(self, seed, mag_w=0.3):
        """The operands of test_stage_a_plane_forms_against_fp64: x ~ N(0, 1), the plane scale (32) and the Gb scale (512) in the columns."""
        rng = np.random.default_rng(seed)
        self.x = rng.standard_normal((self.n_x, self.ldx)).astype(np.float32)
        self.poison()
        for n8, widths in self.prods:
            gcp = sum(widths)
            self.Wv.append((rng.standard_normal((self.k, n8, gcp, 8)) * mag_w * 32.0).astype(np.float32))
            self.Wb.append((rng.standard_normal((self.k, gcp)) * mag_w * 512.0).astype(np.float32))
        return self

    def rhs(self):
        return [R.build_rhs(wv, wb, p[1], self.ncols, self.fmt) for wv, wb, p in zip(self.Wv, self.Wb, self.prods)]

    def covered(self, b):
        """Floats of a row of product b that are plane groups or Gb words: everything else is padding."""
        n8, widths = self.prods[b]
        gcp, per = sum(widths), (8 if self.fmt != 1 else 6)
        m = np.zeros(self.ld, dtype=bool)
        m[:per * n8 * gcp] = True
        c = np.arange(gcp)
        m[(8 * n8 * gcp + c) if self.fmt != 1 else (6 * (n8 * gcp + c // 6) + c % 6)] = True
        return m


def _launch(case, mode=None):
    """The words stage A wrote [nb, n_x, ld] (float32 bytes, NaN pattern where it wrote nothing) and range_flag."""
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import packing as P
    from diffdock_pocket_amd.launch import stream
    lib = L.load()
    dev = torch.device("cuda:0")
    fmt, dw = FORMS[case.form]
    dw = dw if mode is None else mode
    nb = len(case.prods)
    W = torch.from_numpy(np.stack(case.rhs()))
    wh = P.split_h2(W, unified_scale=P.GH_SW).to(dev)           # (split on the host: what test_stage_a_ref64_cpu.py checks)
    xd, Wd = torch.from_numpy(case.x).to(dev), W.to(dev)
    dest = torch.from_numpy(np.stack([R.dest_table(case.ncols, n8 * sum(w), fmt) for n8, w in case.prods])).contiguous().to(dev)
    out = torch.full((nb, case.n_x, case.ld), float("nan"), device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    rows_d = None if case.rows is None else torch.tensor(case.rows, dtype=torch.int32, device=dev)
    cnt_d = None if case.count is None else torch.tensor([case.count], dtype=torch.int32, device=dev)
    nrows = case.n_x if case.rows is None else len(case.rows)
    fn = lib.ddp_stage_a_gh3 if fmt == 1 else lib.ddp_stage_a_gh
    with (_Form(lib, dw) if fmt == 1 else contextlib.nullcontext()):
        L.check(fn(xd.data_ptr(), case.ldx, nrows, None if rows_d is None else rows_d.data_ptr(), None if cnt_d is None else cnt_d.data_ptr(),
                   case.n_x, (C.c_int32 * nb)(*case.offs), nb, Wd.data_ptr(), wh.data_ptr(), case.k, case.ncols, out.data_ptr(), case.ld,
                   flag.data_ptr(), dest.data_ptr(), stream()), "ddp_stage_a_gh")
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(flag.item())


def _untouched(case, words_b):
    """Rows that are not live keep the sentinel in every word of the product's slice."""
    dead = ~case.live
    assert bool((words_b[dead] == SENTINEL).all()), "a row outside the list was written"


def _against_fp64(case, tag, mode=None):
    """Bound (a): every live row holds the fp64 product of ITS OWN x row at ITS OWN row index, inside the forms' bounds; Gb inside the
    product's; padding is the product of zero columns; rows not listed are untouched."""
    out, flag = _launch(case, mode)
    assert flag == 0
    lr = np.flatnonzero(case.live)
    worst_v = worst_b = 0.0
    for b, (n8, widths) in enumerate(case.prods):
        words = out[b].view(np.int32)
        _untouched(case, words)
        if lr.size == 0:
            continue
        V, Gb = decode_gh_rows(torch.from_numpy(np.ascontiguousarray(out[b][lr])), widths, 8 * n8, case.fmt)
        V, Gb = V.numpy(), Gb.numpy()
        assert np.isfinite(V).all() and np.isfinite(Gb).all()
        k, off = case.k, case.offs[b]
        gcp = sum(widths)
        exV, scV = R.product64(case.x[lr], case.Wv[b].reshape(k, -1), off, k)
        exV, scV = exV.reshape(-1, n8, gcp, 8), scV.reshape(-1, n8, gcp, 8)
        exB, scB = R.product64(case.x[lr], case.Wb[b], off, k)
        bound = 2.0 ** -20 * scV + (2.0 ** -25 if case.fmt != 1 else 2.0 ** -19 * np.abs(exV) + 2.0 ** -24)
        rv = float((np.abs(V - exV) / bound).max())
        rb = float((np.abs(Gb - exB) / (2.0 ** -20 * scB)).max())
        worst_v, worst_b = max(worst_v, rv), max(worst_b, rb)
        pad = ~case.covered(b)
        assert not words[lr][:, pad].any(), "a padding word of a written row is not +0"
    print(f"\nstage_a_fp64 {tag:<44s} {case.form:<11s} planes {worst_v:.3f}  Gb {worst_b:.3f}")
    assert worst_v <= 1.0 and worst_b <= 1.0, (tag, case.form, worst_v, worst_b)


# ---- a. bound against fp64, ragged shapes

@pytest.mark.parametrize("nrows", [1, 31, 32, 33, 65, 129, 257])
@pytest.mark.parametrize("form", THREE)
def test_rows_at_tile_and_workgroup_edges(form, nrows):
    """The 32-row tile, the 64 / 128 / 256-row workgroup ranges and one row past each; three products at offsets 0 / 60 / 120."""
    _against_fp64(Case(form, nrows, 184, [0, 60, 120], 60, PRODS3).random(100 + nrows), f"rows={nrows}")


@pytest.mark.parametrize("k", [32, 24, 16])
@pytest.mark.parametrize("form", THREE)
def test_the_other_inner_sizes(form, k):
    """K = 32 / 24 / 16: one or two 16-deep steps, 24 with k padding inside its last one; x beyond a window is NaN (columns 16 + k .. 63)."""
    _against_fp64(Case(form, 65, 64, [0, 16], k, PRODS3[:2]).random(200 + k), f"K={k}")


@pytest.mark.parametrize("ldx,off", [(181, 60), (184, 61)])
@pytest.mark.parametrize("form", THREE)
def test_x_rows_that_are_not_16_byte_aligned(form, ldx, off):
    """An odd row stride / an odd column offset: the 4-byte fetch of x, dense and through a row list."""
    _against_fp64(Case(form, 65, ldx, [0, off, 2 * off], 60, PRODS3).random(300 + ldx), f"ldx={ldx},off={off},dense")
    rows = np.random.default_rng(6).permutation(100)[:65].tolist()
    _against_fp64(Case(form, 100, ldx, [off, 2 * off], 60, PRODS3[:2], rows=rows).random(301 + ldx), f"ldx={ldx},off={off},listed")


@pytest.mark.parametrize("form", THREE)
def test_row_list_unsorted_with_repeats(form):
    """257 entries into 300 rows: a listed row is written at rows[i], not at i, from x row rows[i]; a repeated row once, with that value."""
    rows = np.random.default_rng(3).integers(0, 300, 257).tolist()
    rows[10] = rows[200] = rows[0]
    case = Case(form, 300, 184, [0, 60, 120], 60, PRODS3, rows=rows).random(400)
    assert 0 < int(case.live.sum()) < 257 and not case.live[:257].all()
    _against_fp64(case, "list=257/300,repeats")


@pytest.mark.parametrize("count", [0, 33, 200])
@pytest.mark.parametrize("form", THREE)
def test_device_side_length_below_capacity(form, count):
    """Only the first `count` entries of a list of capacity 257 are live: the rows behind them stay untouched (their x rows are NaN)."""
    rows = np.random.default_rng(4).permutation(300)[:257].tolist()
    _against_fp64(Case(form, 300, 184, [60], 60, PRODS3[:1], rows=rows, count=count).random(500 + count), f"list count={count}/257")


@pytest.mark.parametrize("form", THREE)
def test_long_list_walks_its_tiles(form):
    """12500 entries, 12400 live: more 128-row ranges than the bounded grid of a listed product has workgroups (96), every workgroup walks."""
    rows = np.random.default_rng(5).permutation(12600)[:12500].tolist()
    ncols = 128 if FORMS[form][0] == 1 else None
    _against_fp64(Case(form, 12600, 184, [60], 60, [(3, [4])], ncols=ncols, rows=rows, count=12400).random(600), "list count=12400/12500")


@pytest.mark.parametrize("form", THREE)
def test_layer3_pair_every_byte_accounted_for(form):
    """The layer-3 pair: 23 x 72 and 23 x 28 plane groups in one launch, Gb and padding of the second product start where the first still has
    planes.  Every word of a written row is a decoded plane group, a compared Gb word or a zero."""
    fmt = FORMS[form][0]
    ncols = 13440 if fmt == 1 else 13344            # gh3_ld(180, 72) / 6 * 8, gh_ld(180, 72)
    _against_fp64(Case(form, 65, 184, [0, 60], 60, [(23, [32, 28, 12]), (23, [28])], ncols=ncols).random(700), "layer 3: 23x72 + 23x28")


@pytest.mark.parametrize("nrows", [4095, 4097])
def test_default_dispatch_across_its_threshold(nrows):
    """ddp_sa_drainwave = 1: the symmetric waves below 4096 dense rows, the store wave from there on - against fp64 it does not matter which."""
    _against_fp64(Case("gh3_default", nrows, 184, [0, 60], 60, [(5, [8]), (4, [8])], ncols=384).random(800 + nrows), f"default,rows={nrows}")


@pytest.mark.parametrize("form", THREE)
def test_small_weight_class_at_a_tile_edge(form):
    """mag_w = 0.02: lo words and continuation bytes near the fp16 subnormal edge, one row past a tile."""
    _against_fp64(Case(form, 33, 184, [0, 60, 120], 60, PRODS3).random(900, mag_w=0.02), "rows=33,mag_w=0.02")


# ---- b. / c. exact operands: one-hot x rows, weights whose unified split has no remainder

def _one_hot_case(form, k, listed, seed, p_of_row=None, n_prod=2):
    """Row i of x is 2^p_i at column off + i % k of EVERY product's window (the windows are disjoint) and 0 elsewhere inside them: the x split
    has no lo part, every product element is ONE exact term 2^p_i W[i % k, column] - two exact fp16 x fp16 products whose fp32 sum is that
    fp32 number -, every k slot of the K instantiation is hit.  p_i <= 0, so that no plane value exceeds the weights' largest."""
    ldx, offs = (184, [0, 60]) if k == 60 else (64, [0, 32])
    offs = offs[:n_prod]
    n_x = 65
    rows = None
    if listed:
        rows = np.random.default_rng(seed).permutation(64)[:39].tolist() + [64]       # unsorted; row 64 in the list's last, partial tile
        rows[7] = rows[20]                                                            # (a repeat)
    case = Case(form, n_x, ldx, offs, k, PRODS3[:n_prod], rows=rows)
    rng = np.random.default_rng(seed + 1)
    p = -(np.arange(n_x) % 4) if p_of_row is None else p_of_row
    case.p = p
    case.x = np.zeros((n_x, ldx), dtype=np.float32)
    for o in offs:
        case.x[np.arange(n_x), o + np.arange(n_x) % k] = np.exp2(p)
    case.poison()
    for n8, widths in case.prods:
        gcp = sum(widths)
        case.Wv.append(R.exact_split_weights(rng, (k, n8, gcp, 8)))
        case.Wb.append(R.exact_split_weights(rng, (k, gcp)))
    return case


def _expected_rows(case, b):
    """encode_gh_rows of the exactly known accumulators of product b, live rows only."""
    n8, widths = case.prods[b]
    lr = np.flatnonzero(case.live)
    s = np.exp2(case.p[lr]).astype(np.float32)
    V32 = case.Wv[b][lr % case.k] * s[:, None, None, None]
    Gb32 = case.Wb[b][lr % case.k] * s[:, None]
    return lr, R.encode_gh_rows(V32, Gb32, widths, 8 * n8, case.fmt, ld=case.ld)


def _byte_for_byte(case, want_flag=0):
    out, flag = _launch(case)
    assert flag == want_flag, (case.form, flag)
    for b in range(len(case.prods)):
        words = out[b].view(np.int32)
        _untouched(case, words)
        lr, want = _expected_rows(case, b)
        got, want = words[lr], want.view(np.int32)
        if not np.array_equal(got, want):
            r, c = np.argwhere(got != want)[0]
            raise AssertionError(f"{case.form} product {b}: row {lr[r]} word {c}: {got[r, c] & 0xffffffff:#010x}, expected "
                                 f"{want[r, c] & 0xffffffff:#010x} ({int((got != want).sum())} words differ)")
    return out


@pytest.mark.parametrize("listed", [False, True], ids=["dense", "listed"])
@pytest.mark.parametrize("k", [60, 32, 24, 16])
@pytest.mark.parametrize("form", THREE)
def test_exact_operands_byte_for_byte(form, k, listed):
    """The written rows are encode_gh_rows of the known accumulators, word for word: hi / lo words, continuation bytes, Gb, padding.  Among
    the plane values, through every k slot and the scales 1, 1/2, 1/4, 1/8: a carry of the 19-bit rounding into the next binade
    (8192 - 2^-9 -> 8192), +-65504 (flag stays 0), and (1 + 2^-10) 2^-13 whose quarter and eighth lie below 2^-14 - the hi word a truncated
    subnormal.  (Weights and products of one-hot rows: stage_a_ref64.exact_split_weights, test_stage_a_ref64_cpu.py.)"""
    case = _one_hot_case(form, k, listed, seed=1000 + k)
    for wv in case.Wv:
        wv[:, 0, 1, 3], wv[:, 1, 2, 0], wv[:, 3, 1, 1], wv[:, 2, 0, 5] = R.EDGE_CARRY, R.EDGE_MAX, -R.EDGE_MAX, R.EDGE_TINY
        wv[:, 1, 3, 6] = -R.EDGE_CARRY
    _byte_for_byte(case)


@pytest.mark.parametrize("listed", [False, True], ids=["dense", "listed"])
@pytest.mark.parametrize("form", THREE)
def test_range_flag_at_its_boundary(form, listed):
    """Row 64 - alone in the last, partial tile, dense and as the last entry of a 40-row list - is the one row at scale 1 (k slot 4; row 4
    shares the slot at scale 1/2).  A plane value of exactly 65504 there leaves range_flag at 0 and is stored exactly; the next fp32 number
    raises it, with either sign.  A Gb value beyond the limit does not: the header's range is that of the PLANE values V (|V| > 65504 raises
    range_flag; the other groups are fp32 columns stored as they are).  An x value whose DDP_GH_SX-fold exceeds 65504 in a fetched column
    raises it; 32752, whose double is 65504, does not."""
    p = -np.ones(65, dtype=np.int64)
    p[64] = 0

    def fresh():
        return _one_hot_case(form, 60, listed, seed=2000, p_of_row=p, n_prod=1)

    case = fresh()
    case.Wv[0][4, 2, 3, 1] = R.EDGE_MAX
    out = _byte_for_byte(case, want_flag=0)
    V, _ = decode_gh_rows(torch.from_numpy(out[0][64:65].copy()), case.prods[0][1], 40, case.fmt)
    assert float(V[0, 2, 3, 1]) == 65504.0
    for v in (R.EDGE_OVER, -R.EDGE_OVER):
        case = fresh()
        case.Wv[0][4, 2, 3, 1] = v
        assert _launch(case)[1] == 1, (form, float(v))
    case = fresh()
    case.Wv[0][4, 2, 3, 1] = R.EDGE_MAX
    case.Wb[0][4, 5] = 98304.0                       # (= 1.5 x 2^16: its half is an fp16 number)
    out = _byte_for_byte(case, want_flag=0)
    _, Gb = decode_gh_rows(torch.from_numpy(out[0][64:65].copy()), case.prods[0][1], 40, case.fmt)
    assert float(Gb[0, 5]) == 98304.0
    for xv, want in ((32752.0, 0), (-32752.0, 0), (40000.0, 1)):
        case = fresh()
        case.Wv[0][7], case.Wb[0][7] = 0.0, 0.0     # the column's weights are zero: only the x split sees the value
        case.x[64, case.offs[0] + 7] = xv
        assert _launch(case)[1] == want, (form, xv)
