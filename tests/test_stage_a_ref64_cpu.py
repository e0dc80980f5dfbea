"""tests/stage_a_ref64.py - the numpy definition of stage A's two plane forms - against itself and against helpers.decode_gh_rows, without a
GPU: the round trips inside the bounds include/ddp_hip.h states, plane form 1 at its edges to the bit, the builders' layouts, and the
precondition of the exact-operand GPU test (packing.split_h2 splits its weights without a remainder)."""
import numpy as np
import pytest
import torch

import stage_a_ref64 as R
from helpers import decode_gh_rows

HID, WIDTHS = 40, [8, 4]            # n8 = 5, two parts, gcp = 12


def _roundtrip(V32, Gb32, fmt, widths=WIDTHS, hid=HID):
    rows = R.encode_gh_rows(V32, Gb32, widths, hid, fmt)
    V, Gb = decode_gh_rows(torch.from_numpy(rows), widths, hid, fmt)
    return rows, V.numpy(), Gb.numpy()


def _values(seed, lo_exp, hi_exp, n=64):
    """fp32 values with random signs and magnitudes log-uniform in [2^lo_exp, 2^hi_exp)."""
    rng = np.random.default_rng(seed)
    shape = (n, 5, 12, 8)
    mag = np.exp2(rng.uniform(lo_exp, hi_exp, size=shape))
    return (mag * np.where(rng.random(shape) < 0.5, -1.0, 1.0)).astype(np.float32), rng.standard_normal((n, 12)).astype(np.float32)


def test_form0_round_trip_within_its_floor():
    """hi + lo carries 22 significant bits: |err| <= 2^-22 |V| (what the 2^-20 sum|x w| of the fp64 tests absorbs), and never more than the
    absolute 2^-25 the same tests add - the floor of a subnormal lo word - wherever that is the larger: below |V| = 0.25, down to the end of
    the fp16 normal range.  (Above 0.25 an absolute 2^-25 cannot hold: a normal lo word of a value in [2^E, 2^(E+1)) resolves 2^(E-22).)"""
    V32, Gb32 = _values(0, -14, -2)
    _, V, Gb = _roundtrip(V32, Gb32, 0)
    assert float(np.abs(V - V32.astype(np.float64)).max()) <= 2.0 ** -25
    assert np.array_equal(Gb, Gb32.astype(np.float64))
    V32, Gb32 = _values(1, -14, 15.99)
    _, V, _ = _roundtrip(V32, Gb32, 0)
    v = V32.astype(np.float64)
    assert bool((np.abs(V - v) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all())


def test_form1_round_trip_within_19_bits():
    V32, Gb32 = _values(2, -20, 15.99)
    _, V, Gb = _roundtrip(V32, Gb32, 1)
    v = V32.astype(np.float64)
    assert bool((np.abs(V - v) <= 2.0 ** -19 * np.abs(v) + 2.0 ** -24).all())
    assert np.array_equal(Gb, Gb32.astype(np.float64))
    big = np.abs(v) >= 2.0 ** -14                                  # (where the byte counts: 19 bits alone, and clearly coarser than two fp16 words)
    assert bool((np.abs(V - v)[big] <= 2.0 ** -19 * np.abs(v)[big]).all())
    assert float((np.abs(V - v)[big] / np.abs(v)[big]).max()) > 2.0 ** -22


def _one(v, fmt=1):
    """The hi word (uint16), the byte and the decoded value of one plane value."""
    V32 = np.zeros((1, 1, 1, 8), dtype=np.float32)
    V32[0, 0, 0, 3] = v
    rows = R.encode_gh_rows(V32, np.zeros((1, 1), dtype=np.float32), [1], 8, fmt)
    raw = rows.view(np.uint8)[0]
    V, _ = decode_gh_rows(torch.from_numpy(rows), [1], 8, fmt)
    other = np.delete(np.arange(24), [6, 7, 19])
    assert not raw[other].any()
    return int(raw[6:8].view(np.uint16)[0]), int(raw[19]), float(V[0, 0, 0, 3])


def test_form1_edges_to_the_bit():
    # the 19-bit rounding carries into the next binade: 2 - 2^-21 -> 2
    assert _one(2.0 - 2.0 ** -21) == (0x4000, 0, 2.0)
    assert _one(-(2.0 - 2.0 ** -21)) == (0xc000, 0, -2.0)
    assert _one(float(R.EDGE_CARRY)) == (0x7000, 0, 8192.0)
    # one unit of the 19th bit below: stays, hi = 1.11..1 (10 bits), byte = 0xff
    assert _one(2.0 - 2.0 ** -18) == (0x3fff, 0xff, 2.0 - 2.0 ** -18)
    # half a unit rounds up by magnitude, less than half rounds down
    assert _one(1.0 + 2.0 ** -19) == (0x3c00, 1, 1.0 + 2.0 ** -18)
    assert _one(1.0 + 2.0 ** -19 - 2.0 ** -23) == (0x3c00, 0, 1.0)
    # hi is a TRUNCATION: 1 + 2^-10 - 2^-18 keeps hi = 1.0 and the byte 0xff (rounding hi to nearest would give 1 + 2^-10)
    assert _one(1.0 + 2.0 ** -10 - 2.0 ** -18) == (0x3c00, 0xff, 1.0 + 2.0 ** -10 - 2.0 ** -18)
    # the largest plane value
    assert _one(65504.0) == (0x7bff, 0, 65504.0)
    assert _one(-65504.0) == (0xfbff, 0, -65504.0)
    # below 2^-14 the hi word is a truncated subnormal and the byte means nothing: decode gives hi alone
    v = float(R.EDGE_TINY) * 0.125                                 # (1 + 2^-10) 2^-16 = 256.25 x 2^-24
    hw, _, dec = _one(v)
    assert hw == 256 and dec == 256 * 2.0 ** -24
    hw, _, dec = _one(-v)
    assert hw == 0x8000 + 256 and dec == -256 * 2.0 ** -24
    hw, b, dec = _one(2.0 ** -14 * (1 - 2.0 ** -12))               # just below the normal range, byte bits set: still hi alone
    assert hw == 0x03ff and b != 0 and dec == 1023 * 2.0 ** -24
    # zeros
    assert _one(0.0) == (0, 0, 0.0)
    hw, b, dec = _one(-0.0)
    assert (hw, b) == (0x8000, 0) and dec == 0.0 and np.signbit(dec)


def test_form0_words():
    """hi = fp16(V) to nearest even, lo = fp16(V - hi): 1 + 2^-10 - 2^-18 -> hi = 1 + 2^-10, lo = -2^-18."""
    V32 = np.zeros((1, 1, 1, 8), dtype=np.float32)
    V32[0, 0, 0, 5] = 1.0 + 2.0 ** -10 - 2.0 ** -18
    raw = R.encode_gh_rows(V32, np.zeros((1, 1), dtype=np.float32), [1], 8, 0).view(np.uint8)[0]
    h = raw[:32].view(np.float16)
    assert float(h[5]) == 1.0 + 2.0 ** -10 and float(h[8 + 5]) == -2.0 ** -18
    assert not np.delete(h, [5, 13]).any()


@pytest.mark.parametrize("fmt", [0, 1])
def test_layout_places(fmt):
    """Unit (part, k8, c) and Gb of padded column c sit where the header says; rows are DDP_GH_LD / DDP_GH3_LD floats, zero elsewhere."""
    n8, gcp = 5, 12
    V32 = np.zeros((1, n8, gcp, 8), dtype=np.float32)
    Gb32 = np.zeros((1, gcp), dtype=np.float32)
    V32[0, 3, 9, 2] = 1.5                 # part 1 (columns 8 .. 11), k8 = 3, c = 1
    Gb32[0, 7] = -3.25
    rows = R.encode_gh_rows(V32, Gb32, WIDTHS, HID, fmt)
    unit = n8 * 8 + 3 * 4 + 1             # units of part 0 + k8 * wp + c
    if fmt == 0:
        assert rows.shape[1] == ((n8 * 8 + 1) * gcp + 31) // 32 * 32 == 512
        h = rows.view(np.float16)[0]
        assert float(h[16 * unit + 2]) == 1.5
        assert float(rows[0, 8 * n8 * gcp + 7]) == -3.25
    else:
        assert rows.shape[1] == (n8 * gcp + 2 + 15) // 16 * 96 == 384
        raw = rows.view(np.uint8)[0]
        assert float(raw[24 * unit + 4:24 * unit + 6].view(np.float16)[0]) == 1.5
        assert float(raw[24 * (n8 * gcp + 1) + 4:24 * (n8 * gcp + 1) + 8].view(np.float32)[0]) == -3.25
    assert np.count_nonzero(rows.view(np.uint16)) == 2     # (1.5: a hi word, lo word / byte 0; -3.25 = 0xc0500000: one nonzero half)


@pytest.mark.parametrize("fmt", [0, 1])
def test_builder_and_dest_table(fmt):
    """build_rhs puts weight (k, k8, c, i) at the product column whose group is the unit's index, Gb where the form stores it; a product
    computed with that right-hand side and regrouped by the dest table is the encoder's input."""
    rng = np.random.default_rng(5)
    k, n8, gcp = 6, 5, 12
    ncols = 1024 if fmt == 0 else 512
    Wv = rng.standard_normal((k, n8, gcp, 8)).astype(np.float32)
    Wb = rng.standard_normal((k, gcp)).astype(np.float32)
    W = R.build_rhs(Wv, Wb, WIDTHS, ncols, fmt)
    unit = n8 * 8 + 3 * 4 + 1
    assert np.array_equal(W[:, 8 * unit:8 * unit + 8], Wv[:, 3, 9])
    assert np.array_equal(W[:, 8 * 2:8 * 2 + 8], Wv[:, 0, 2])
    gbc = R.gb_columns(n8, gcp, fmt)
    assert np.array_equal(W[:, gbc], Wb) and len(set(gbc.tolist())) == gcp and int(gbc.min()) == 8 * n8 * gcp
    assert np.count_nonzero(W) == np.count_nonzero(Wv) + np.count_nonzero(Wb)
    if fmt == 1:                          # product columns 3 and 7 of an fp32 group are not stored: nothing may sit there
        assert not W[:, 8 * n8 * gcp + 3::8].any() and not W[:, 8 * n8 * gcp + 7::8].any()
        assert gbc[:7].tolist() == [480, 481, 484, 485, 482, 486, 488]
    tab = R.dest_table(ncols, n8 * gcp, fmt)
    assert tab.shape == (ncols // 8, 2) and tab.dtype == np.int32
    assert bool((tab[:n8 * gcp, 0] & 1).all()) and not (tab[n8 * gcp:, 0] & 1).any()
    per = 8 if fmt == 0 else 6
    assert np.array_equal(tab[:, 0] & ~1, per * np.arange(ncols // 8)) and np.array_equal(tab[:, 1], per * np.arange(ncols // 8) + 4)
    # the same table as the library's own, from the plane-group count alone
    from diffdock_pocket_amd import packing as P
    assert np.array_equal(tab, P.gh_dest_table(WIDTHS, n8, ncols, fmt=fmt).numpy())
    p64, s64 = R.product64(np.eye(k, 9, 2), W, 2, k)
    assert np.array_equal(p64, W.astype(np.float64)) and np.array_equal(s64, np.abs(W).astype(np.float64))


def test_split_h2_is_exact_on_the_exact_operand_weights():
    """The precondition of test_gpu_stage_a_planes_fp64's byte-for-byte cases: packing.split_h2(W, unified_scale = GH_SW) on a CPU tensor
    leaves hi + lo == W GH_SW in fp64, lo a normal fp16 number or zero, for exact_split_weights and for the edge values; and every weight
    (k, column) sits at plane word [k / 16][k / 8 % 2][column][k % 8]."""
    from diffdock_pocket_amd import packing as P
    assert P.GH_SW == R.GH_SW
    rng = np.random.default_rng(7)
    for k in (60, 32, 24, 16):
        W = R.exact_split_weights(rng, (2, k, 64))
        W[0, :, 5], W[0, :, 6], W[0, :, 7], W[1, :, 8], W[1, :, 9] = R.EDGE_CARRY, R.EDGE_MAX, R.EDGE_OVER, R.EDGE_TINY, 0.0
        assert int(np.unique(np.abs(W)).size) > 0.9 * W.size
        wh = P.split_h2(torch.from_numpy(W), unified_scale=P.GH_SW)
        kp = (k + 15) // 16 * 16
        assert wh.dtype == torch.float16 and tuple(wh.shape) == (2, 2, kp // 16, 2, 64, 8)
        planes = wh.permute(0, 1, 2, 3, 5, 4).reshape(2, 2, kp, 64).double().numpy()        # [nb, plane, k, column]
        assert np.array_equal(planes[:, 0, :k] + planes[:, 1, :k], W.astype(np.float64) * R.GH_SW)
        assert not planes[:, :, k:].any()
        lo = np.abs(planes[:, 1, :k])
        assert bool(((lo == 0) | (lo >= 2.0 ** -14)).all()) and float((lo > 0).mean()) > 0.5
        hi = planes[:, 0, :k]
        assert bool(((hi == 0) == (W == 0)).all()) and bool((np.abs(hi[hi != 0]) >= 2.0 ** -14).all())
