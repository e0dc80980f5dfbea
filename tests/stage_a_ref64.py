"""The definition of stage A's plane forms (ddp_stage_a_gh: form 0, ddp_stage_a_gh3: form 1) in numpy, CPU only: what a G row IS, byte for
byte, written from the text of include/ddp_hip.h (ddp_conv_task_t::gh, gh_fmt, DDP_GH_SX, DDP_ROWS_S*, ddp_stage_a_gh, ddp_stage_a_gh3) and
from nothing else - not from packing.gh_dest_table, not from the kernels.  tests/test_stage_a_ref64_cpu.py checks it against itself and
against helpers.decode_gh_rows (its inverse); tests/test_gpu_stage_a_planes_fp64.py holds every kernel form against it.

A product's columns are ordered [part][k8][c < wp][8 k's] (8-column PLANE GROUPS, n8 * gcp of them, gcp = the sum of the part widths),
then the Gb columns, then zero padding.  In both forms group g of the product leaves at a place that depends on g alone:
  form 0   a plane group at byte 32 g of the row: 8 fp16 hi words fp16(V), then 8 fp16 lo words fp16(V - hi); the other groups are 8 fp32
           columns at float 8 g - Gb of padded column c at float 8 n8 gcp + c;
  form 1   every group at byte 24 g: a plane group as 8 fp16 hi words + 8 continuation bytes, an fp32 group as SIX values - product columns
           0, 1, 4, 5, 2, 6 of the group, in that order - so Gb of padded column c sits at byte 24 (n8 gcp + c / 6) + 4 (c % 6)."""
import numpy as np

GH_SX = 2.0                          # DDP_GH_SX: the kernel splits x at this scale, the weight planes are those of w / DDP_GH_SX
GH_SW = 1.0 / GH_SX
FP32_COLS = (0, 1, 4, 5, 2, 6)       # form 1: product column (inside its 8-column group) of the j-th fp32 value the group stores
V_LIMIT = 65504.0                    # |V| beyond it raises range_flag in both forms


def product64(x, W, off, k):
    """(x[:, off:off + k] @ W, |x[:, off:off + k]| @ |W|) in fp64: the product and the scale of its rounding-error bounds."""
    xs = np.asarray(x, dtype=np.float64)[:, off:off + k]
    W = np.asarray(W, dtype=np.float64)
    assert xs.shape[1] == k and W.shape[0] == k
    return xs @ W, np.abs(xs) @ np.abs(W)


def row_floats(ncols, fmt):
    """Floats of an output row that a product of `ncols` columns writes: all of them in form 0, 6 per 8-column group in form 1."""
    assert ncols % 8 == 0
    return ncols if fmt != 1 else ncols // 8 * 6


def gb_columns(n8, gcp, fmt):
    """Product column of Gb of padded column c = 0 .. gcp - 1."""
    c = np.arange(gcp)
    if fmt != 1:
        return 8 * n8 * gcp + c
    return 8 * (n8 * gcp + c // 6) + np.asarray(FP32_COLS)[c % 6]


def build_rhs(Wv, Wb, widths, ncols, fmt):
    """The right-hand side [k, ncols] of one product in the product's column order: Wv [k, n8, gcp, 8] the plane weights (k8 group, padded
    column of the slot, k slot of the group), Wb [k, gcp] the Gb weights; every other column is zero (padding)."""
    Wv, Wb = np.asarray(Wv, dtype=np.float32), np.asarray(Wb, dtype=np.float32)
    k, n8, gcp, _ = Wv.shape
    assert sum(widths) == gcp and Wb.shape == (k, gcp)
    gbc = gb_columns(n8, gcp, fmt)
    assert ncols % 8 == 0 and int(gbc.max()) < ncols
    W = np.zeros((k, ncols), dtype=np.float32)
    cum = 0
    for w in widths:                                                      # part p: a contiguous tile [k8][c < wp][8]
        W[:, 8 * n8 * cum:8 * n8 * (cum + w)] = Wv[:, :, cum:cum + w].reshape(k, -1)
        cum += w
    W[:, gbc] = Wb
    return W


def dest_table(ncols, nplane, fmt):
    """dest[g][0..1] of one product from its plane-group count alone: the float offsets inside the row of group g's two 16-byte pieces, bit 0
    of [g][0] set = a plane group.  Form 0: hi words at byte 32 g, lo words behind them; an fp32 group at float 8 g.  Form 1: group g at
    byte 24 g (only the bit is read)."""
    g = np.arange(ncols // 8, dtype=np.int64)
    per = 8 if fmt != 1 else 6
    tab = np.stack([per * g, per * g + 4], axis=1).astype(np.int32)
    assert 0 <= nplane <= ncols // 8
    tab[:nplane, 0] += 1
    return tab


def _rtz_f16(v32):
    """fp32 -> fp16 by TRUNCATION of the magnitude (fp16 subnormals included; beyond the range: the largest fp16 number)."""
    v = np.asarray(v32, dtype=np.float32)
    bits = v.view(np.uint32)
    normal = (bits & np.uint32(0xffffe000)).view(np.float32).astype(np.float64)      # 10 mantissa bits kept
    sub = np.trunc(v.astype(np.float64) * 2.0 ** 24) * 2.0 ** -24                    # multiples of 2^-24 below 2^-14
    a = np.abs(v.astype(np.float64))
    t = np.where(a >= 2.0 ** -14, normal, sub)
    t = np.where(a > V_LIMIT, np.copysign(V_LIMIT, v.astype(np.float64)), t)
    h = t.astype(np.float16)
    assert np.array_equal(h.astype(np.float64), t)                                   # (the cast rounded nothing; -0 stays -0)
    return h


def split_form0(V32):
    """(hi, lo) fp16 words of form 0: hi = fp16(V), lo = fp16(V - hi), round to nearest even."""
    V = np.asarray(V32, dtype=np.float32)
    hi = V.astype(np.float16)
    rest = V.astype(np.float64) - hi.astype(np.float64)
    r32 = rest.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), rest)       # V - hi is an fp32 number: the kernel's fp32 subtraction is exact
    return hi, r32.astype(np.float16)


def split_form1(V32):
    """(hi fp16, u8) of form 1: V rounded to 19 significant bits by magnitude - half a unit of the 19th bit added to the fp32 bit pattern,
    so that a carry runs into the exponent -, hi = that value truncated to fp16, u8 = its next eight mantissa bits."""
    V = np.ascontiguousarray(V32, dtype=np.float32)
    b = V.view(np.uint32) + np.uint32(0x10)                   # bits 4 .. 0 of the 23-bit mantissa lie below the 19th significant bit
    r = (b & np.uint32(0xffffffe0)).view(np.float32)
    return _rtz_f16(r), ((b >> np.uint32(5)) & np.uint32(0xff)).astype(np.uint8)


def encode_gh_rows(V32, Gb32, widths, hid, fmt, ld=None):
    """fp32 plane values V32 [N, n8, gcp, 8] and fp32 Gb values Gb32 [N, gcp] -> the G rows [N, ld] float32 (bytes) of plane form `fmt`:
    the inverse of helpers.decode_gh_rows.  ld defaults to DDP_GH_LD / DDP_GH3_LD; whatever is neither a plane group nor a Gb word is the
    product of zero columns: +0."""
    V = np.ascontiguousarray(V32, dtype=np.float32)
    Gb = np.ascontiguousarray(Gb32, dtype=np.float32)
    n8, gcp = (hid + 7) // 8, sum(widths)
    N = V.shape[0]
    assert V.shape == (N, n8, gcp, 8) and Gb.shape == (N, gcp)
    if ld is None:
        ld = ((n8 * 8 + 1) * gcp + 31) // 32 * 32 if fmt != 1 else (n8 * gcp + (gcp + 5) // 6 + 15) // 16 * 96
    raw = np.zeros((N, 4 * ld), dtype=np.uint8)
    cum = 0
    for w in widths:
        Vp = V[:, :, cum:cum + w]                                                     # [N, n8, w, 8]: unit (k8, c) of the part
        if fmt != 1:
            hi, lo = split_form0(Vp)
            unit = np.stack([hi.view(np.uint16), lo.view(np.uint16)], axis=3)         # [N, n8, w, plane, 8] halves
            base = 32 * n8 * cum
            raw[:, base:base + 32 * n8 * w] = np.ascontiguousarray(unit).view(np.uint8).reshape(N, -1)
        else:
            hi, u8 = split_form1(Vp)
            unit = np.concatenate([np.ascontiguousarray(hi).view(np.uint8).reshape(N, n8, w, 16), u8], axis=3)
            base = 24 * n8 * cum
            raw[:, base:base + 24 * n8 * w] = unit.reshape(N, -1)
        cum += w
    f32 = raw.view(np.float32)
    c = np.arange(gcp)
    if fmt != 1:
        assert 8 * n8 * gcp + gcp <= ld
        f32[:, 8 * n8 * gcp + c] = Gb
    else:
        assert 6 * (n8 * gcp + (gcp + 5) // 6) <= ld
        f32[:, 6 * (n8 * gcp + c // 6) + c % 6] = Gb
    return f32


def exact_split_weights(rng, shape):
    """fp32 weights W whose unified planes at GH_SW are EXACT with a normal (or zero) lo word: W GH_SW = H + L, H an fp16 number in
    [2^8, 2^14), L = j 2^(E(H) - 22) with |j| < 2048 - less than half a unit of H's last place, so that fp16(W GH_SW) = H, and itself an fp16
    number of at least 2^-14.  21 - 23 significant bits: the 19-bit rounding of form 1 has work to do on every one of them."""
    e = rng.integers(8, 14, size=shape)
    H = np.ldexp(1.0 + rng.integers(0, 1024, size=shape) / 1024.0, e)
    j = rng.integers(-2047, 2048, size=shape) * (rng.random(size=shape) < 0.85)
    W = (H + np.ldexp(j.astype(np.float64), e - 22)) * np.where(rng.random(size=shape) < 0.5, -1.0, 1.0) / GH_SW
    W32 = W.astype(np.float32)
    assert np.array_equal(W32.astype(np.float64), W)
    return W32


# plane values at the edges of form 1, as weights (V = the weight itself under a one-hot x row of 1.0); each is exact under the GH_SW split
EDGE_CARRY = np.float32(8192.0 - 2.0 ** -9)          # = 2^12 (2 - 2^-21): the 19-bit rounding carries into the next binade (8192)
EDGE_MAX = np.float32(65504.0)                       # the largest plane value
EDGE_OVER = np.nextafter(np.float32(65504.0), np.float32(np.inf))      # 65504 + 2^-8: the first value that raises range_flag
EDGE_TINY = np.float32((1.0 + 2.0 ** -10) * 2.0 ** -13)                # x 2^-3 it lies below 2^-14: the hi word is a truncated subnormal
