"""The kernels AROUND the conv, each against the definition in include/ddp_hip.h evaluated in float64 on the CPU, element by element,
at ragged shapes and degenerate inputs: ddp_segment_reduce, ddp_node_linear, the score-norm lookups of ddp_trrot_head / ddp_tor_head,
ddp_torsion_sh, ddp_knn, the radius searches and ddp_pose_update.

Every test builds seeded inputs, calls the kernel through the C ABI (diffdock_pocket_amd._lib / launch wrappers) and compares with
numpy float64.  No kernel of the library serves as reference for another one (bitwise comparisons of two FORMS of one kernel are
extra assertions, never the definition).  Tolerances are derived in the docstrings from the inputs; the one measured number is the
device sinf / cosf error of ddp_node_linear (see _sin_yardstick; profiles/kernel_fp64_tests.txt).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from helpers import SENTINEL, _assert_within, _bits, _up

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23
U24 = 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda")


def _api():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import launch as K
    return L, L.load(), K


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ====================================================================================================== 1. ddp_segment_reduce
_EDGE_PATTERN = (0, 1, 7, 8, 9, 16, 17)     # per-node edge counts on the edges of the kernel's 8-row load groups


def _edge_counts(rng, n_nodes, big):
    if n_nodes == 1:
        return np.array([9], dtype=np.int64)
    cnt = np.resize(np.array(_EDGE_PATTERN, dtype=np.int64), n_nodes)
    rng.shuffle(cnt)
    if big and n_nodes > 4:
        cnt[n_nodes // 2] = 1003                 # one node with ~1000 incoming edges
    cnt[0] = 0                                   # the FIRST and the LAST node are empty
    cnt[-1] = 0
    return cnt


class _Src:
    pass


def _make_src(rng, n_nodes, d_out, dev, rowmap="none", count="none", big=True, misalign_msg=False):
    """One incoming conv of a reduce problem.  rowmap: none | identity | perm (messages stored permuted) | compact (several CSR
    positions share one stored row).  count: none | cap (*n_edges_dev = capacity) | below (capacity 37 rows beyond the count, the
    rows behind the count are NaN and never listed by rowptr) | zero (*n_edges_dev = 0: contributes exactly 0)."""
    s = _Src()
    cnt = _edge_counts(rng, n_nodes, big)
    s.cnt = cnt
    s.rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    E = int(s.rowptr[-1])
    s.scale = ((rng.random(d_out) + 0.5) * rng.choice([-1.0, 1.0], d_out)).astype(np.float32)
    s.shift = rng.standard_normal(d_out).astype(np.float32)
    rm = None
    if rowmap == "compact":
        U = max(1, E // 3)
        stored = rng.standard_normal((U, d_out)).astype(np.float32)
        rm = rng.integers(0, U, E).astype(np.int32)
        s.msg = stored[rm]                       # the message of CSR position p
    else:
        s.msg = rng.standard_normal((E, d_out)).astype(np.float32)
        stored = s.msg
        if rowmap == "identity":
            rm = np.arange(E, dtype=np.int32)
        elif rowmap == "perm":
            rm = rng.permutation(E).astype(np.int32)
            stored = np.empty_like(s.msg)
            stored[rm] = s.msg
    s.n_edges, s.live, cnt_dev = E, True, None
    if count == "cap":
        cnt_dev = E
    elif count == "zero":
        cnt_dev, s.live = 0, False
    elif count == "below":
        cnt_dev, s.n_edges = E, E + 37
        if rm is None:
            stored = np.concatenate([stored, np.full((37, d_out), np.nan, np.float32)])
        else:
            rm = np.concatenate([rm, np.zeros(37, np.int32)])
    flat = torch.empty(stored.size + 4, device=dev)
    off = 1 if misalign_msg else 0               # a view that starts 4 bytes into the 256-byte aligned allocation
    s.d_msg = flat[off:off + stored.size].view(stored.shape)
    s.d_msg.copy_(torch.from_numpy(stored))
    s.d_rowptr, s.d_scale, s.d_shift = _up(s.rowptr, dev), _up(s.scale, dev), _up(s.shift, dev)
    s.d_rowmap = _up(rm, dev) if rm is not None else None
    s.d_cnt = torch.tensor([cnt_dev], dtype=torch.int32, device=dev) if cnt_dev is not None else None
    return s


def _empty_src():
    """A conv the HOST drops (n_edges == 0): no array of it may be read, so it carries none."""
    s = _Src()
    s.n_edges, s.live = 0, False
    s.d_msg = s.d_rowptr = s.d_scale = s.d_shift = s.d_rowmap = s.d_cnt = None
    return s


def _src_update64(s, n_nodes, d_out):
    """(update, bound term) of one source in float64: mean_p msg * scale + shift and (cnt + 3) (sum_p |msg| / max(cnt, 1) |scale| + |shift|)."""
    upd, bnd = np.zeros((n_nodes, d_out)), np.zeros((n_nodes, d_out))
    if not s.live:
        return upd, bnd
    m = s.msg.astype(np.float64)
    seg, ab = np.zeros((n_nodes, d_out)), np.zeros((n_nodes, d_out))
    nz = s.cnt > 0
    if nz.any():                                 # (starts of the non-empty segments: reduceat sums up to the next start / the end)
        starts = s.rowptr[:-1][nz].astype(np.int64)
        seg[nz] = np.add.reduceat(m, starts, axis=0)
        ab[nz] = np.add.reduceat(np.abs(m), starts, axis=0)
    den = np.maximum(s.cnt, 1)[:, None].astype(np.float64)
    sc, sh = s.scale.astype(np.float64), s.shift.astype(np.float64)
    upd = seg / den * sc + sh
    bnd = (s.cnt[:, None] + 3.0) * (ab / den * np.abs(sc) + np.abs(sh))
    return upd, bnd


def _x_buffer(rng, rows, ldx, d_out, dev, misalign=False):
    host = rng.standard_normal((rows, ldx)).astype(np.float32)
    host[:, d_out:] = SENTINEL
    flat = torch.empty(rows * ldx + 4, device=dev)
    off = 1 if misalign else 0
    x = flat[off:off + rows * ldx].view(rows, ldx)
    x.copy_(torch.from_numpy(host))
    return x, host


def _reduce(x, ldx, n_nodes, d_out, srcs, accumulate, n_rep=1, rep_stride=0, nsrc=None):
    L, lib, K = _api()
    arr = (L.ReduceSrc * max(len(srcs), 1))()
    for i, s in enumerate(srcs):
        arr[i].msg, arr[i].rowptr = K._p(s.d_msg), K._p(s.d_rowptr)
        arr[i].bn_scale, arr[i].bn_shift, arr[i].n_edges = K._p(s.d_scale), K._p(s.d_shift), s.n_edges
        arr[i].rowmap, arr[i].n_edges_dev = K._p(s.d_rowmap), K._p(s.d_cnt)
    return lib.ddp_segment_reduce(C.c_void_p(x.data_ptr()), ldx, n_nodes, d_out, arr, len(srcs) if nsrc is None else nsrc,
                                  1 if accumulate else 0, n_rep, rep_stride, K.stream())


def _check_reduce(x, x_old, srcs, n_nodes, d_out, accumulate, n_rep, rep_stride, what):
    """The header's definition in float64 and the forward bound
        |got - want| <= 2^-23 sum_k (cnt_k + 3) (sum_p |msg| / max(cnt_k, 1) |scale| + |shift|) + 2^-23 nsrc |x_old|
    with nsrc = the sources that contribute (one dropped by the host or by a zero device-side count adds nothing, not even a rounding)
    (in-order fp32 sum of cnt terms, one division, one multiply-add - contracted or not -, the residual adds; unit roundoff 2^-24,
    factor 2 for the uncertainty about contraction).  Everything the definition does not name - columns [d_out, ldx), the rows
    between n_nodes and rep_stride - keeps its bits."""
    got = x.detach().cpu().numpy()
    want = x_old.astype(np.float64).copy()
    tol = np.zeros_like(want)
    named = np.zeros(want.shape, dtype=bool)
    upd, bnd = np.zeros((n_nodes, d_out)), np.zeros((n_nodes, d_out))
    for s in srcs:
        u, b = _src_update64(s, n_nodes, d_out)
        upd += u
        bnd += b
    for g in range(n_rep if n_rep > 1 else 1):
        r0 = g * rep_stride if n_rep > 1 else 0
        old = x_old[r0:r0 + n_nodes, :d_out].astype(np.float64) if (accumulate or n_rep > 1) else np.zeros((n_nodes, d_out))
        want[r0:r0 + n_nodes, :d_out] = old + upd
        tol[r0:r0 + n_nodes, :d_out] = U23 * bnd + U23 * sum(1 for s in srcs if s.live) * np.abs(old)
        named[r0:r0 + n_nodes, :d_out] = True
    assert np.array_equal(_bits(got)[~named], _bits(x_old)[~named]), f"{what}: an element outside x[n, :d_out] changed"
    _assert_within(got[named], want[named], tol[named], what)


def _three_sources(rng, n_nodes, d_out, dev, big=True):
    return [_make_src(rng, n_nodes, d_out, dev, "none", "none", big),
            _make_src(rng, n_nodes, d_out, dev, "compact", "below", False),
            _make_src(rng, n_nodes, d_out, dev, "perm", "cap", False)]


def _sweep(rng, dev, n_nodes, d_out, ldxs, nsrcs, big, what):
    sources = _three_sources(rng, n_nodes, d_out, dev, big)
    combo = 0
    for ldx in ldxs:
        for nsrc in nsrcs:
            for accumulate in (0, 1):
                for n_rep in (1, 5):
                    srcs = [sources[(combo + i) % 3] for i in range(nsrc)]
                    rep_stride = n_nodes + 3 if n_rep > 1 else 0
                    rows = n_rep * rep_stride if n_rep > 1 else n_nodes
                    x, x_old = _x_buffer(rng, rows, ldx, d_out, dev)
                    assert _reduce(x, ldx, n_nodes, d_out, srcs, accumulate, n_rep, rep_stride) == 0
                    _check_reduce(x, x_old, srcs, n_nodes, d_out, accumulate, n_rep, rep_stride,
                                  f"{what} ldx={ldx} nsrc={nsrc} acc={accumulate} n_rep={n_rep}")
                    combo += 1


@pytest.mark.parametrize("d_out", [1, 3, 36, 42, 90, 180, 1024])
def test_segment_reduce_matches_its_fp64_definition(d_out):
    """x[n, :d_out] (+)= sum_k (mean_p msg_k[rowmap_k[p]] * bn_scale_k + bn_shift_k) for ldx in {d_out, d_out rounded up to 4, 184}
    (the 4-channel form runs where d_out and ldx are multiples of 4, the 1-channel form elsewhere - 42 and 90 are the layer 0 -> 1
    widths of the shipped models), 1 - 3 sources with different edge sets (plain storage / a compacted array behind a row map with
    a device-side count below the capacity / permuted storage with a count equal to the capacity), accumulate 0 / 1, n_rep 1 / 5
    with rep_stride > n_nodes.  Per-node edge counts 0, 1, 7, 8, 9, 16, 17, one node with 1003, first and last node empty."""
    dev = _dev()
    rng = np.random.default_rng(1000 + d_out)
    n_nodes = 23
    ldxs = sorted(v for v in {d_out, (d_out + 3) // 4 * 4, 184} if v >= d_out)
    probe = _edge_counts(np.random.default_rng(0), n_nodes, True)
    assert set(_EDGE_PATTERN) <= set(probe.tolist()) and probe[0] == 0 and probe[-1] == 0 and probe.max() == 1003
    _sweep(rng, dev, n_nodes, d_out, ldxs, (1, 2, 3), True, f"segment_reduce d_out={d_out}")


@pytest.mark.parametrize("d_out", [3, 4, 12])
@pytest.mark.parametrize("n_nodes", [1, 255, 256, 257])
def test_segment_reduce_where_a_block_of_items_crosses_nodes(n_nodes, d_out):
    """Small d_out with 1 / 255 / 256 / 257 nodes: the 4-channel form's 256 (node, channel quad) items per workgroup end inside a
    node (d_out = 12: three quads per node) or exactly on one (d_out = 4); d_out = 3 is the 1-channel form at the same sizes."""
    dev = _dev()
    rng = np.random.default_rng(7 * n_nodes + d_out)
    _sweep(rng, dev, n_nodes, d_out, sorted({d_out, (d_out + 3) // 4 * 4}), (2,), False, f"segment_reduce n={n_nodes} d_out={d_out}")


@pytest.mark.parametrize("d_out,n_nodes", [(36, 23), (180, 23), (4, 257), (12, 257)])
def test_segment_reduce_forms_agree_bitwise(d_out, n_nodes):
    """Bitwise equal on one problem: the 4-channel and the 1-channel form (the latter reached by handing x, or msg, as a view that
    starts 4 bytes into a 16-byte aligned buffer - the host's own predicate: d_out, ldx multiples of 4 and x, msg, bn_scale,
    bn_shift 16-byte aligned); an identity row map and none; permuted storage behind a row map and plain storage."""
    assert "DDP_REDUCE_NARROW" not in os.environ, "the diagnostic variable forces one form: both must run here"
    dev = _dev()
    ldx = d_out + 4
    for accumulate in (0, 1):
        for n_rep in (1, 5):
            rep_stride = n_nodes + 2 if n_rep > 1 else 0
            rows = n_rep * rep_stride if n_rep > 1 else n_nodes
            results = {}
            for form in ("wide", "narrow_x", "narrow_msg", "identity", "perm"):
                rng = np.random.default_rng(31 * d_out + n_nodes)      # the same problem for every form
                a = _make_src(rng, n_nodes, d_out, dev, "none", "none", big=(n_nodes < 100))
                b = _make_src(rng, n_nodes, d_out, dev, "none", "cap", big=False)
                x, x_old = _x_buffer(rng, rows, ldx, d_out, dev, misalign=(form == "narrow_x"))
                if form != "wide":
                    rng2 = np.random.default_rng(5)
                    a2 = _make_src(np.random.default_rng(31 * d_out + n_nodes), n_nodes, d_out, dev,
                                   {"identity": "identity", "perm": "none"}.get(form, "none"), "none", big=(n_nodes < 100),
                                   misalign_msg=(form == "narrow_msg"))
                    assert np.array_equal(a2.msg, a.msg) and np.array_equal(a2.rowptr, a.rowptr)
                    if form == "perm":                                # the same messages, stored permuted behind a row map
                        perm = rng2.permutation(a.n_edges).astype(np.int32)
                        stored = np.empty_like(a.msg)
                        stored[perm] = a.msg
                        a2.d_msg, a2.d_rowmap = _up(stored, dev), _up(perm, dev)
                    a = a2
                aligned = x.data_ptr() % 16 == 0 and all(t.data_ptr() % 16 == 0 for s in (a, b) for t in (s.d_msg, s.d_scale, s.d_shift))
                assert aligned == (form not in ("narrow_x", "narrow_msg")) and d_out % 4 == 0 and ldx % 4 == 0
                assert _reduce(x, ldx, n_nodes, d_out, [a, b], accumulate, n_rep, rep_stride) == 0
                _check_reduce(x, x_old, [a, b], n_nodes, d_out, accumulate, n_rep, rep_stride, f"forms[{form}] d_out={d_out} n={n_nodes}")
                results[form] = x.detach().cpu().numpy().copy()
            for form, r in results.items():
                assert _same_bits(r, results["wide"]), f"{form} differs from the 4-channel form (acc={accumulate}, n_rep={n_rep})"


def test_segment_reduce_device_counts_and_dropped_sources():
    """*n_edges_dev = 0 and n_edges = 0 on the host both contribute exactly 0: the same bits as the launch without that source
    (and the fp64 definition); with every source empty accumulate = 1 leaves x alone and accumulate = 0 writes zeros."""
    dev = _dev()
    n_nodes, d_out, ldx = 23, 36, 40
    for accumulate in (0, 1):
        res = {}
        for case in ("left_out", "dev_zero", "host_empty"):
            rng = np.random.default_rng(77)
            a = _make_src(rng, n_nodes, d_out, dev, "none", "none")
            c = _make_src(rng, n_nodes, d_out, dev, "compact", "below", big=False)
            x, x_old = _x_buffer(rng, n_nodes, ldx, d_out, dev)
            mid = {"dev_zero": _make_src(np.random.default_rng(3), n_nodes, d_out, dev, "perm", "zero", big=False),
                   "host_empty": _empty_src()}.get(case)
            srcs = [a, c] if mid is None else [a, mid, c]
            assert _reduce(x, ldx, n_nodes, d_out, srcs, accumulate) == 0
            _check_reduce(x, x_old, srcs, n_nodes, d_out, accumulate, 1, 0, f"reduce[{case}] acc={accumulate}")
            res[case] = x.detach().cpu().numpy().copy()
        assert _same_bits(res["dev_zero"], res["left_out"]) and _same_bits(res["host_empty"], res["left_out"])
        rng = np.random.default_rng(78)
        z = [_make_src(rng, n_nodes, d_out, dev, "none", "zero", big=False), _make_src(rng, n_nodes, d_out, dev, "identity", "zero", big=False)]
        x, x_old = _x_buffer(rng, n_nodes, ldx, d_out, dev)
        assert _reduce(x, ldx, n_nodes, d_out, z, accumulate) == 0
        want = x_old.copy()
        if not accumulate:
            want[:, :d_out] = 0.0
        assert _same_bits(x, want)


def test_segment_reduce_two_launches_against_one():
    """Two accumulate launches of one source each and one launch of two sources are NOT required to be bitwise equal: (x + a) + b
    against x + (a + b) - the header fixes no association of the residual adds, and a kernel may form the sources' sum first.
    So this pair is held to the fp64 definition with the derived bound only: the one launch against (x_old; a, b), the two
    launches step by step (the second one's x_old is what the first one wrote)."""
    dev = _dev()
    n_nodes, d_out, ldx = 23, 90, 92
    rng = np.random.default_rng(11)
    a = _make_src(rng, n_nodes, d_out, dev, "none", "none")
    b = _make_src(rng, n_nodes, d_out, dev, "compact", "cap", big=False)
    x, x_old = _x_buffer(rng, n_nodes, ldx, d_out, dev)
    assert _reduce(x, ldx, n_nodes, d_out, [a, b], 1) == 0
    _check_reduce(x, x_old, [a, b], n_nodes, d_out, 1, 1, 0, "one launch, two sources")
    x.copy_(torch.from_numpy(x_old))
    assert _reduce(x, ldx, n_nodes, d_out, [a], 1) == 0
    _check_reduce(x, x_old, [a], n_nodes, d_out, 1, 1, 0, "two launches, first")
    x_mid = x.detach().cpu().numpy().copy()
    assert _reduce(x, ldx, n_nodes, d_out, [b], 1) == 0
    _check_reduce(x, x_mid, [b], n_nodes, d_out, 1, 1, 0, "two launches, second")


def test_segment_reduce_refuses_what_it_cannot_run():
    """nsrc = 4, d_out = 0 / 1025 and rep_stride < n_nodes with n_rep > 1: an error code, and no element of x is written."""
    dev = _dev()
    n_nodes, d_out, ldx = 23, 36, 40
    rng = np.random.default_rng(5)
    srcs = [_make_src(rng, n_nodes, d_out, dev, big=False) for _ in range(4)]
    x, x_old = _x_buffer(rng, 5 * n_nodes, ldx, d_out, dev)
    assert _reduce(x, ldx, n_nodes, d_out, srcs, 1) != 0
    assert _reduce(x, ldx, n_nodes, 0, srcs[:1], 1) != 0
    assert _reduce(x, 1028, 1, 1025, srcs[:1], 1) != 0
    assert _reduce(x, ldx, n_nodes, d_out, srcs[:2], 1, n_rep=5, rep_stride=n_nodes - 1) != 0
    assert _reduce(x, ldx, n_nodes, d_out, srcs[:2], 0, n_rep=2, rep_stride=0) != 0
    torch.cuda.synchronize()
    assert _same_bits(x, x_old)


# ====================================================================================================== 2. ddp_node_linear
_SIN_T_GRID = 4096          # the tests' diffusion times are multiples of 1 / 4096: the yardstick below covers every argument they use
_SIN_SCALES = (1000.0, 10000.0)


def _freq(sd):
    half = sd // 2
    return np.exp(np.arange(half, dtype=np.float32) * np.float32(-(math.log(10000.0) / (half - 1)))).astype(np.float32)


def _sin_args(t32, scale, freq32):
    """The float32 argument of the embedding in the reference's order: (scale * t) * freq[k], both products rounded to float32."""
    st = (np.float32(scale) * t32.astype(np.float32)).astype(np.float32)
    return (st[:, None] * freq32[None, :]).astype(np.float32)


_YARDSTICK = {}


def _sin_yardstick(dev):
    """max |torch.sin / torch.cos (ROCm, float32) - float64 sin / cos| over every argument the node-linear tests can form:
    t = i / 4096, embedding_scale 1000 and 10000, the 16 frequencies of sd = 32 / 33 (arguments up to 1e4).  torch-ROCm is the
    library ddp_node_linear's in-kernel sinf / cosf replaced; the kernel is allowed TWICE this (another, equally valid range
    reduction).  The yardstick itself is held to <= 2^-23 (1.19e-7).  Measured on an MI355X: 6.58e-8 (the kernel is then allowed 1.32e-7; its own error there: 6.2e-8; profiles/kernel_fp64_tests.txt)."""
    if "v" not in _YARDSTICK:
        t = (np.arange(_SIN_T_GRID + 1, dtype=np.float64) / _SIN_T_GRID).astype(np.float32)
        worst = 0.0
        for scale in _SIN_SCALES:
            a = _sin_args(t, scale, _freq(32))
            ad = _up(a, dev)
            worst = max(worst, float(np.abs(torch.sin(ad).cpu().numpy().astype(np.float64) - np.sin(a.astype(np.float64))).max()),
                        float(np.abs(torch.cos(ad).cpu().numpy().astype(np.float64) - np.cos(a.astype(np.float64))).max()))
        # the allowance must not grow unnoticed with another torch build: one float32 ulp of values in [1/2, 1) bounds the yardstick
        assert worst <= 2.0 ** -23, f"torch-ROCm sin / cos is off by {worst:.3e} > 2^-23: no yardstick for the kernel's sinf / cosf"
        _YARDSTICK["v"] = worst
        print(f"[fp64] sin / cos yardstick (torch-ROCm float32 against float64): {worst:.3e}")
    return _YARDSTICK["v"]


class _NodeCase:
    pass


def _node_case(rng, dev, n_rows, ncols, emb_mode=0, n_cat=0, emb_dim=0, dense=(), sd=0, sigma="t", t_stride=1, scale=1000.0,
               sig_out=False, bias=True, add=False, zero_to=0, pad=3):
    """One ddp_node_job_t on seeded inputs of the model's magnitudes with its float64 definition.  Every leading dimension is
    `pad` wider than the used width; the padding columns of the INPUTS are NaN (a kernel that reads one shows it), those of the
    outputs hold SENTINEL.  zero_to: 0 | an int >= ncols | "ld" (= ld_out)."""
    L, lib, K = _api()
    c = _NodeCase()
    c.keep = []

    def up(a):
        t = _up(a, dev)
        c.keep.append(t)
        return t

    def padded(a):
        return np.concatenate([a, np.full((a.shape[0], pad), np.nan, np.float32)], 1) if pad else a

    j = L.NodeJob()
    j.n_rows, j.ncols = n_rows, ncols
    segs, segs_abs = [], []                        # the K segments of the A row (float64) and their |.| for the bound
    emb = emb_abs = None
    if emb_mode:
        dims = [int(v) for v in rng.integers(2, 9, n_cat)]
        offs = np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(np.int64)
        table = (rng.standard_normal((sum(dims), emb_dim)) * 0.5).astype(np.float32)
        cat = np.stack([rng.integers(0, d, n_rows) for d in dims], 1).astype(np.int32)
        cat[0] = 0 if n_rows > 1 else [(d - 1) * (f & 1) for f, d in enumerate(dims)]      # the first row of every table ...
        cat[-1] = [d - 1 for d in dims] if n_rows > 1 else cat[-1]                          # ... and the last one
        cat_p = np.concatenate([cat, np.zeros((n_rows, 2), np.int32)], 1)
        rows = cat.astype(np.int64) + offs[None, :]
        emb = table.astype(np.float64)[rows].sum(1)
        emb_abs = np.abs(table.astype(np.float64))[rows].sum(1)
        j.cat, j.ld_cat, j.n_cat, j.table, j.emb_dim, j.emb_mode = up(cat_p).data_ptr(), cat_p.shape[1], n_cat, up(table).data_ptr(), emb_dim, emb_mode
        for f, o in enumerate(offs):
            j.feat_off[f] = int(o)
        if emb_mode == 1:
            segs.append(emb)
            segs_abs.append(emb_abs)
    for d, n in enumerate(dense):
        a = rng.standard_normal((n_rows, n)).astype(np.float32)
        j.dense[d], j.ld_dense[d], j.n_dense[d] = up(padded(a)).data_ptr(), n + pad, n
        segs.append(a.astype(np.float64))
        segs_abs.append(np.abs(a.astype(np.float64)))
    c.sd, c.sin_rows, c.want_sig, c.sig_exact = sd, None, None, True
    k_sig0 = sum(s.shape[1] for s in segs)
    if sd and sigma == "emb":
        a = rng.standard_normal((n_rows, sd)).astype(np.float32)
        j.sig_emb, j.ld_sig, j.sd = up(padded(a)).data_ptr(), sd + pad, sd
        c.want_sig = a.astype(np.float64)
        segs.append(c.want_sig)
        segs_abs.append(np.abs(c.want_sig))
    elif sd:
        half = sd // 2
        freq = _freq(sd)
        nt = n_rows if t_stride else 1
        t = (rng.integers(0, _SIN_T_GRID + 1, nt) / _SIN_T_GRID).astype(np.float32)
        arg = _sin_args(t if t_stride else np.repeat(t, n_rows), scale, freq).astype(np.float64)
        c.want_sig = np.concatenate([np.sin(arg), np.cos(arg), np.zeros((n_rows, sd - 2 * half))], 1)
        j.t, j.t_stride, j.scale, j.freq, j.sd = up(t).data_ptr(), t_stride, scale, up(freq).data_ptr(), sd
        c.sig_exact = False
        c.sin_rows = (k_sig0, k_sig0 + 2 * half)          # rows of w that multiply a device sinf / cosf value
        segs.append(c.want_sig)
        segs_abs.append(np.abs(c.want_sig))
    A = np.concatenate(segs, 1) if segs else np.zeros((n_rows, 0))
    A_abs = np.concatenate(segs_abs, 1) if segs_abs else np.zeros((n_rows, 0))
    c.K = A.shape[1]
    w = (rng.standard_normal((max(c.K, 1), ncols)) * 0.3).astype(np.float32)[:c.K]
    j.w = up(w if c.K else np.zeros((1, ncols), np.float32)).data_ptr()
    w64 = w.astype(np.float64)
    want = A @ w64
    mag = A_abs @ np.abs(w64)
    if bias:
        b = rng.standard_normal(ncols).astype(np.float32)
        j.bias = up(b).data_ptr()
        want = want + b
        mag = mag + np.abs(b)
    if emb_mode == 2:
        want = want + emb[:, :ncols]
        mag = mag + emb_abs[:, :ncols]
    if add:
        a = rng.standard_normal((n_rows, ncols)).astype(np.float32)
        j.add, j.ld_add = up(padded(a)).data_ptr(), ncols + pad
        want = want + a
        mag = mag + np.abs(a.astype(np.float64))
    c.want, c.mag = want, mag
    c.sin_w = np.abs(w64[c.sin_rows[0]:c.sin_rows[1]]).sum(0) if c.sin_rows else np.zeros(ncols)
    if zero_to == "ld":
        ld_out = zero_to = ncols + 5
    else:
        ld_out = max(ncols, zero_to) + pad + 2
    c.zero_to, c.ld_out, c.ncols, c.n_rows = zero_to, ld_out, ncols, n_rows
    c.out = torch.empty(max(n_rows, 1), ld_out, device=dev)
    j.out, j.ld_out, j.zero_to = c.out.data_ptr(), ld_out, zero_to
    c.sig_out = None
    if sig_out and sd:
        c.sig_out = torch.empty(max(n_rows, 1), sd + 4, device=dev)
        j.sig_out, j.ld_sig_out = c.sig_out.data_ptr(), sd + 4
    c.job = j
    _node_reset(c)
    return c


def _node_reset(c):
    c.out.fill_(float(SENTINEL))
    if c.sig_out is not None:
        c.sig_out.fill_(float(SENTINEL))


def _node_launch(cases):
    L, lib, K = _api()
    arr = (L.NodeJob * max(len(cases), 1))(*[c.job for c in cases])
    return lib.ddp_node_linear(arr, len(cases), K.stream())


def _node_check(c, dev, what):
    """out[n, :ncols] against the header's formula in float64 with
        |got - want| <= (K + 2) 2^-24 sum_k |a_k| |w_k| + eps_sin sum_{sigma rows k} |w_k|
    where the sum over k runs over EVERY term that is added into the element: the K products of the fp32 FMA chain (an embedding
    column a_k counted with the sum of the |table entries| it is made of) and the bias, pass-through embedding and `add` terms
    of the epilogue (weight 1).  eps_sin = 2 x the measured torch-ROCm sin / cos error (_sin_yardstick); zero for a handed-over
    sig_emb.  Columns [ncols, zero_to) are +0.0, everything behind keeps SENTINEL; sig_out[:, :sd] is the embedding (exact copy
    of sig_emb, or within eps_sin of float64 sin / cos; the trailing column of an odd sd exactly 0)."""
    n, nc = c.n_rows, c.ncols
    got = c.out.detach().cpu().numpy()
    if n == 0:
        assert (_bits(got) == _bits(np.full_like(got, SENTINEL))).all(), f"{what}: an n_rows = 0 job wrote something"
        return
    eps_sin = 0.0 if c.sig_exact else 2.0 * _sin_yardstick(dev)
    tol = (c.K + 2) * U24 * c.mag + eps_sin * c.sin_w[None, :]
    _assert_within(got[:n, :nc], c.want, tol, what)
    zt = max(c.zero_to, nc)
    assert (_bits(got[:n, nc:zt]) == 0).all(), f"{what}: columns [ncols, zero_to) are not +0.0"
    assert (_bits(got[:n, zt:]) == _bits(np.full_like(got[:n, zt:], SENTINEL))).all(), f"{what}: a column behind zero_to was written"
    if c.sig_out is not None:
        gs = c.sig_out.detach().cpu().numpy()
        sd = c.sd
        if c.sig_exact:
            assert np.array_equal(_bits(gs[:n, :sd]), _bits(c.want_sig.astype(np.float32))), f"{what}: sig_out is not a copy of sig_emb"
        else:
            _assert_within(gs[:n, :sd], c.want_sig, np.full(c.want_sig.shape, eps_sin), what + " sig_out")
            if sd & 1:
                assert (_bits(gs[:n, sd - 1]) == 0).all(), f"{what}: the padding column of an odd sd is not 0"
        assert (_bits(gs[:n, sd:]) == _bits(np.full_like(gs[:n, sd:], SENTINEL))).all(), f"{what}: sig_out behind sd was written"


# K on the edges of the kernel's 128-wide chunks, built from different segment mixes: 127, 128, 129 and the receptor encoder's 1404
_K_SPECS = {127: dict(emb_mode=1, n_cat=3, emb_dim=16, dense=(79,), sd=32),
            128: dict(dense=(96,), sd=32),
            129: dict(dense=(64, 33), sd=32),      # the second chunk is ONE live column (the last cos), no zero padding behind it
            1404: dict(emb_mode=1, n_cat=5, emb_dim=92, dense=(1280,), sd=32)}


@pytest.mark.parametrize("K", [127, 128, 129, 1404])
@pytest.mark.parametrize("n_rows", [1, 31, 32, 33, 1000])
def test_node_linear_rows_and_k_on_the_tile_edges(n_rows, K):
    """n_rows around the 32-row workgroup tile x K around the 128-wide chunk (one and two dense parts with ld_dense > n_dense,
    the sinusoidal part evaluated in the kernel; every K ends in a live column - K = 129 is a second chunk of exactly one), ncols
    cycling through 1, 16, 60, 255, 256.  Odd sd: test_node_linear_options."""
    dev = _dev()
    rng = np.random.default_rng(10 * n_rows + K)
    ncols = [1, 16, 60, 255, 256][([1, 31, 32, 33, 1000].index(n_rows) + [127, 128, 129, 1404].index(K)) % 5]
    c = _node_case(rng, dev, n_rows, ncols, sig_out=True, scale=_SIN_SCALES[K & 1], **_K_SPECS[K])
    assert c.K == K
    assert _node_launch([c]) == 0
    _node_check(c, dev, f"node_linear n_rows={n_rows} K={K} ncols={ncols}")


_NODE_OPTION_CASES = {
    "mode0_nobias_add": dict(n_rows=33, ncols=60, dense=(50,), sd=32, bias=False, add=True, zero_to=0),
    "mode1_zero_to_ncols": dict(n_rows=31, ncols=16, emb_mode=1, n_cat=16, emb_dim=24, sd=32, zero_to=16, sig_out=True),
    "mode2_wide_table": dict(n_rows=70, ncols=60, emb_mode=2, n_cat=4, emb_dim=77, dense=(32,), sd=0, zero_to=184),
    "mode2_two_dense_zero_to_ld": dict(n_rows=33, ncols=255, emb_mode=2, n_cat=2, emb_dim=256, dense=(60, 130), sd=0, zero_to="ld"),
    "sig_emb_given_odd": dict(n_rows=40, ncols=256, dense=(17,), sd=33, sigma="emb", sig_out=True, add=True),
    "sig_emb_given_even": dict(n_rows=32, ncols=1, sd=32, sigma="emb", sig_out=True, zero_to=9),
    "t_stride0": dict(n_rows=65, ncols=60, dense=(8,), sd=32, t_stride=0, scale=10000.0, sig_out=True),
    "t_stride0_odd_sd": dict(n_rows=1, ncols=16, sd=33, t_stride=0, sig_out=True, bias=False),
    "sigma_only_sd0_dense": dict(n_rows=1000, ncols=255, dense=(128,), sd=0, add=True, zero_to=260),
    "sigma_columns_only": dict(n_rows=257, ncols=60, sd=32, scale=10000.0, zero_to="ld"),
}


@pytest.mark.parametrize("name", list(_NODE_OPTION_CASES))
def test_node_linear_options(name):
    """The three emb_modes (2 with emb_dim > ncols), bias NULL, add with ld_add > ncols, zero_to = 0 / ncols / ld_out / between,
    sig_emb given against computed, t_stride 0 against 1, odd sd, sig_out with ld_sig_out > sd, 16 categorical features with
    values at the first and the last row of every table."""
    dev = _dev()
    rng = np.random.default_rng(sorted(_NODE_OPTION_CASES).index(name))
    c = _node_case(rng, dev, **_NODE_OPTION_CASES[name])
    assert _node_launch([c]) == 0
    _node_check(c, dev, f"node_linear[{name}]")


def test_node_linear_eight_jobs_in_one_launch_equal_single_launches():
    """Eight jobs of different shapes - one of them with n_rows = 0 - in ONE launch: every job within its fp64 bound, and bitwise
    what eight single-job launches write."""
    dev = _dev()
    rng = np.random.default_rng(8)
    specs = [dict(n_rows=1000, ncols=60, **_K_SPECS[1404]), dict(n_rows=1, ncols=1, dense=(3,), sd=0),
             dict(n_rows=0, ncols=16, dense=(8,), sd=32), dict(n_rows=33, ncols=255, sig_out=True, **_K_SPECS[129]),
             dict(n_rows=32, ncols=256, emb_mode=2, n_cat=3, emb_dim=256, dense=(20,), sd=0, zero_to="ld"),
             dict(n_rows=95, ncols=16, sd=32, t_stride=0, sig_out=True, zero_to=20), dict(n_rows=64, ncols=60, sd=33, sigma="emb", add=True),
             dict(n_rows=31, ncols=60, bias=False, **_K_SPECS[127])]
    cases = [_node_case(rng, dev, **s) for s in specs]
    single = []
    for i, c in enumerate(cases):
        assert _node_launch([c]) == 0
        _node_check(c, dev, f"node_linear single job {i}")
        single.append((c.out.detach().cpu().numpy().copy(), c.sig_out.detach().cpu().numpy().copy() if c.sig_out is not None else None))
        _node_reset(c)
    assert _node_launch(cases) == 0
    for i, (c, (o, s)) in enumerate(zip(cases, single)):
        _node_check(c, dev, f"node_linear job {i} of 8")
        assert _same_bits(c.out, o) and (s is None or _same_bits(c.sig_out, s)), f"job {i}: one launch of 8 differs from its own launch"


def test_node_linear_refuses_what_it_cannot_run():
    """ncols = 257, zero_to < ncols, emb_mode = 2 with a table narrower than the output, 9 jobs: an error code, nothing written."""
    dev = _dev()
    rng = np.random.default_rng(9)
    ok = dict(n_rows=5, dense=(8,), sd=0)
    wide = _node_case(rng, dev, ncols=256, **ok)
    wide.job.ncols = 257
    low = _node_case(rng, dev, ncols=16, zero_to=20, **ok)
    low.job.zero_to = 15
    narrow = _node_case(rng, dev, ncols=16, emb_mode=2, n_cat=2, emb_dim=16, **ok)
    narrow.job.emb_dim = 15
    for c, what in ((wide, "ncols = 257"), (low, "zero_to < ncols"), (narrow, "emb_mode 2 with a narrow table")):
        assert _node_launch([c]) != 0, what
    nine = [_node_case(rng, dev, ncols=16, **ok) for _ in range(9)]
    assert _node_launch(nine) != 0
    torch.cuda.synchronize()
    for c in [wide, low, narrow] + nine:
        assert (_bits(c.out) == _bits(np.full(tuple(c.out.shape), SENTINEL))).all()


# ====================================================================================================== 3. score-norm lookups
SO3_N, SO3_LO, SO3_HI = 1000, math.log10(0.01), math.log10(2.0)           # utils/so3.py: MIN_EPS, MAX_EPS, N_EPS
TORUS_N, TORUS_LO, TORUS_HI = 5000, math.log(3e-3), math.log(2.0)         # utils/torus.py: SIGMA_MIN, SIGMA_MAX, SIGMA_N
PI32 = np.float32(np.pi)
N_SWEEP = 8192


def _so3_index32(sigma32, lo32, span32, n):
    """utils/so3.py:85-89 in float32: round (half to even), THEN clip to [0, n - 1]."""
    x = (np.log10(sigma32.astype(np.float32)) - np.float32(lo32)) / np.float32(span32) * np.float32(n)
    assert x.dtype == np.float32
    return np.clip(np.around(x).astype(np.int64), 0, n - 1)


def _torus_index32(sigma32, lo32, span32, n):
    """utils/torus.py:78-82 in float32: clip to [0, n], THEN round (half to even)."""
    x = np.log(sigma32.astype(np.float32) / PI32)
    x = (x - np.float32(lo32)) / np.float32(span32) * np.float32(n)
    assert x.dtype == np.float32
    return np.round(np.clip(x, np.float32(0), np.float32(n))).astype(np.int64)


def _index64(sigma32, lo32, span32, n, torus):
    s = sigma32.astype(np.float64)
    lg = np.log(s / float(PI32)) if torus else np.log10(s)
    return (lg - float(np.float32(lo32))) / float(np.float32(span32)) * n


def _neighbour_bins(x64, n_hi):
    """The two bins a sigma may select when its float64 index lies within 1e-3 of a half-integer (device log10f / logf may differ
    from numpy's by an ulp); equal where it does not (also wherever both sides of the half-way point clamp to the same end)."""
    a = np.clip(np.rint(x64 - 1e-3), 0, n_hi).astype(np.int64)
    b = np.clip(np.rint(x64 + 1e-3), 0, n_hi).astype(np.int64)
    return a, b


def _sweep_sigmas(lo_sigma, hi_sigma, lo_log, span_log, n, bin0, base10, unit, seed):
    """N_SWEEP float32 sigmas: log-spaced from half the table's lower end to twice its upper end (both clamps; a seeded sub-bin
    offset of the spacing), the two exact ends, the 64 exact bin centres from bin0 on and the float32 values nearest to the 64
    half-way points between them.  unit: sigma = unit * base^(lo + span i / n)."""
    def at(i):
        e = lo_log + span_log * np.asarray(i, dtype=np.float64) / n
        return unit * (10.0 ** e if base10 else np.exp(e))
    n_log = N_SWEEP - 2 - 128
    jitter = np.random.default_rng(seed).random()
    grid = (np.arange(n_log) + jitter) / n_log
    logs = np.exp(np.log(0.5 * lo_sigma) + grid * (np.log(2.0 * hi_sigma) - np.log(0.5 * lo_sigma)))
    s = np.concatenate([logs, [lo_sigma, hi_sigma], at(bin0 + np.arange(64)), at(bin0 + np.arange(64) + 0.5)]).astype(np.float32)
    assert s.shape == (N_SWEEP,)
    return s


def _expected_bins(sigma32, lo32, span32, n, n_hi, torus, what):
    """CPU only, BEFORE the launch: the numpy float32 index of every sigma, its two admissible bins (equal but for the sigmas whose
    float64 index lies within 1e-3 of a half-way point) and the conditions on the sweep itself: at most 1 % of it takes the
    exemption (64 of the ~77 are the deliberately placed half-way points, ~13 = 0.2 % of the log-spaced ones: close to the cap by
    construction), every bin of the table's range and both clamps are reached."""
    want = (_torus_index32 if torus else _so3_index32)(sigma32, lo32, span32, n)
    a, b = _neighbour_bins(_index64(sigma32, lo32, span32, n, torus), n_hi)
    exempt = a != b
    assert exempt.mean() <= 0.01, f"{what}: {exempt.sum()} of {exempt.size} sigmas would be exempt (cap 1 %): reseed the spacing"
    assert ((want == a) | exempt).all(), f"{what}: the float32 and the float64 index disagree away from a half-way point"
    assert want.min() == 0 and want.max() == n_hi and len(np.unique(want)) > 0.9 * n_hi, f"{what}: the sweep misses bins or a clamp"
    return want, a, b


def _check_swept_bins(got, sigma32, expected, what):
    """Every sigma must select the numpy float32 index, except the exempt ones (_expected_bins): they may select either neighbour."""
    want, a, b = expected
    exempt = a != b
    strict = ~exempt
    bad = strict & (got != want)
    assert not bad.any(), (f"{what}: {bad.sum()} sigmas select another bin than numpy float32, first: sigma {sigma32[bad][0]!r} "
                           f"got {got[bad][0]} want {want[bad][0]}")
    bad = exempt & (got != a) & (got != b)
    assert not bad.any(), f"{what}: {bad.sum()} half-way sigmas select neither neighbouring bin"
    print(f"[fp64] {what}: {strict.sum()} exact, {exempt.sum()} half-way ({100 * exempt.mean():.2f} %), bins hit {len(np.unique(got))}")


def _trrot_lookup(dev, sigma32, table32, so3_n, lo32, span32):
    """ddp_trrot_head with an MLP that returns exactly 1 (w1 = 0, b1 = 1, w2 one-hot, b2 = 0) and the rot vector (0, 1, 0): the y
    component of the rot output IS the selected table entry."""
    L, lib, K = _api()
    B, ns, sd = sigma32.shape[0], 4, 2
    gp = np.zeros((B, 14), np.float32)
    gp[:, 0], gp[:, 4] = 1.0, 1.0                   # tr = (1, 0, 0), rot = (0, 1, 0): |v| = 1 exactly
    one_hot = np.zeros(ns, np.float32)
    one_hot[1] = 1.0
    t = dict(gp=_up(gp, dev), emb=torch.randn(B, sd, device=dev), w1=torch.zeros(ns, 1 + sd, device=dev), b1=torch.ones(ns, device=dev),
             w2=_up(one_hot, dev), b2=torch.zeros(1, device=dev), sig=_up(sigma32, dev), tab=_up(table32, dev),
             out_tr=torch.empty(B, 3, device=dev), out_rot=torch.empty(B, 3, device=dev))
    r = L.TrRotArgs()
    r.gp, r.ld_gp, r.n_graphs, r.ns, r.sd, r.graph_emb = t["gp"].data_ptr(), 14, B, ns, sd, t["emb"].data_ptr()
    for h in range(2):
        r.w1[h], r.b1[h], r.w2[h], r.b2[h] = t["w1"].data_ptr(), t["b1"].data_ptr(), t["w2"].data_ptr(), t["b2"].data_ptr()
    r.sigma[1] = t["sig"].data_ptr()
    r.so3_table, r.so3_n, r.so3_lo, r.so3_span = t["tab"].data_ptr(), so3_n, float(np.float32(lo32)), float(np.float32(span32))
    r.out[0], r.out[1] = t["out_tr"].data_ptr(), t["out_rot"].data_ptr()
    L.check(lib.ddp_trrot_head(C.byref(r), K.stream()), "ddp_trrot_head")
    rot, tr = t["out_rot"].cpu().numpy(), t["out_tr"].cpu().numpy()
    assert np.array_equal(tr, np.tile(np.float32([1, 0, 0]), (B, 1))) and not rot[:, [0, 2]].any()
    return rot[:, 1]


def _tor_lookup(dev, sigma32, table32, torus_n, lo32, span32):
    """ddp_tor_head with ns = 1, h = (1, 1), w1 = (10, 10), w2 = 1: the pre-norm value is tanh(20) = 1 to the last bit or the one
    before, so out[b] = sqrt(table[index]) (1 - at most 2^-24); bond b reads the sigma of graph perm[b]."""
    L, lib, K = _api()
    T = sigma32.shape[0]
    perm = np.random.default_rng(1).permutation(T).astype(np.int32)
    h = np.full((T, 4), np.nan, np.float32)
    h[:, :2] = 1.0
    t = dict(h=_up(h, dev), w1=_up(np.float32([10, 10]), dev), w2=_up(np.float32([1]), dev), sig=_up(sigma32, dev), gob=_up(perm, dev),
             tab=_up(table32, dev), out=torch.empty(T, device=dev))
    q = L.TorArgs()
    q.h, q.ld_h, q.n_bonds, q.ns, q.w1, q.w2 = t["h"].data_ptr(), 4, T, 1, t["w1"].data_ptr(), t["w2"].data_ptr()
    q.sigma, q.graph_of_bond = t["sig"].data_ptr(), t["gob"].data_ptr()
    q.torus_table, q.torus_n, q.torus_lo, q.torus_span = t["tab"].data_ptr(), torus_n, float(np.float32(lo32)), float(np.float32(span32))
    q.out = t["out"].data_ptr()
    L.check(lib.ddp_tor_head(C.byref(q), K.stream()), "ddp_tor_head")
    out = np.empty(T, np.float32)
    out[perm] = t["out"].cpu().numpy()               # back to the order of the sigmas
    return out


def test_so3_score_norm_lookup_swept_over_the_whole_table():
    """sigma_rot over the 1000 bins of the so3 table, both clamped ends, 64 exact bin centres and the 64 half-way points between
    them: the selected INDEX (table[i] = i + 1; one spare entry behind the table that a correct kernel never reads) equals
    utils/so3.py:85-89 evaluated with numpy in float32."""
    dev = _dev()
    lo32, span32 = np.float32(SO3_LO), np.float32(SO3_HI - SO3_LO)
    sig = _sweep_sigmas(0.01, 2.0, SO3_LO, SO3_HI - SO3_LO, SO3_N, 300, True, 1.0, seed=0)
    table = np.arange(1, SO3_N + 2, dtype=np.float32)
    expected = _expected_bins(sig, lo32, span32, SO3_N, SO3_N - 1, False, "so3 score norm")
    got = _trrot_lookup(dev, sig, table, SO3_N, lo32, span32)
    assert np.array_equal(got, np.rint(got)) and got.min() >= 1
    _check_swept_bins(got.astype(np.int64) - 1, sig, expected, "so3 score norm")


def test_torus_score_norm_lookup_swept_over_the_whole_table():
    """sigma_tor over the 5001 entries of the torus table in the same way (table[i] = (i + 1)^2, the kernel multiplies by its
    square root): utils/torus.py:78-82 in float32 - clip to [0, n], then round."""
    dev = _dev()
    lo32, span32 = np.float32(TORUS_LO), np.float32(TORUS_HI - TORUS_LO)
    sig = _sweep_sigmas(3e-3 * math.pi, 2.0 * math.pi, TORUS_LO, TORUS_HI - TORUS_LO, TORUS_N, 2000, False, math.pi, seed=0)
    table = (np.arange(1, TORUS_N + 3, dtype=np.float64) ** 2).astype(np.float32)
    expected = _expected_bins(sig, lo32, span32, TORUS_N, TORUS_N, True, "torus score norm")
    got = _tor_lookup(dev, sig, table, TORUS_N, lo32, span32)
    assert np.abs(got - np.rint(got)).max() < 0.01 and got.min() > 0.5, "the output is not the square root of a table entry"
    _check_swept_bins(np.rint(got).astype(np.int64) - 1, sig, expected, "torus score norm")


def test_score_norm_lookups_round_half_to_even():
    """Exact ties, independent of the device logarithm: log10(1) = 0 and ln(pi32 / pi32) = 0 exactly, so with lo = -(k + 0.5),
    span = n = 64 the float32 index argument IS k + 0.5.  numpy rounds half to even (k + 0.5 -> k for even k, k + 1 for odd k)."""
    dev = _dev()
    n = 64
    for k in range(12):
        lo32, span32 = np.float32(-(k + 0.5)), np.float32(64.0)
        want = k if k % 2 == 0 else k + 1
        s = np.float32([1.0])
        assert _so3_index32(s, lo32, span32, n)[0] == want
        got = _trrot_lookup(dev, s, np.arange(1, n + 2, dtype=np.float32), n, lo32, span32)
        assert int(got[0]) - 1 == want, f"so3 tie at {k}.5: bin {int(got[0]) - 1}, numpy {want}"
        s = np.array([PI32], np.float32)
        assert _torus_index32(s, lo32, span32, n)[0] == want
        got = _tor_lookup(dev, s, (np.arange(1, n + 3, dtype=np.float64) ** 2).astype(np.float32), n, lo32, span32)
        assert int(np.rint(got[0])) - 1 == want, f"torus tie at {k}.5: bin {int(np.rint(got[0])) - 1}, numpy {want}"


def test_trrot_head_with_a_zero_vector_in_one_graph():
    """|v| = 0 for the translation part of one graph: the expression the kernel replaces, tr / |tr| * MLP(..) / sigma
    (all_atom_score_model.py:362-384), is 0 / 0 = NaN for that row.  The kernel gives NaN there too; the row's rotation output and
    every other row are bitwise what they are when that graph's vector is not zero (one workgroup per graph)."""
    L, lib, K = _api()
    dev = _dev()
    rng = np.random.default_rng(4)
    B, ns, sd, bad = 5, 16, 32, 2
    w = {k: _up(rng.standard_normal(s).astype(np.float32), dev) for k, s in (("w1", (2, ns, 1 + sd)), ("b1", (2, ns)), ("w2", (2, ns)), ("b2", (2, 1)))}
    emb, sig = _up(rng.standard_normal((B, sd)).astype(np.float32), dev), _up((rng.random((2, B)) + 0.2).astype(np.float32), dev)
    table = _up(np.arange(1, SO3_N + 1, dtype=np.float32), dev)
    gp_ok = rng.standard_normal((B, 12)).astype(np.float32)
    gp_zero = gp_ok.copy()
    gp_zero[bad, 6:9] = -gp_zero[bad, 0:3]            # 1o + 1e halves cancel exactly: tr = 0
    outs = {}
    for name, gp in (("ok", gp_ok), ("zero", gp_zero)):
        gpd, o_tr, o_rot = _up(gp, dev), torch.empty(B, 3, device=dev), torch.empty(B, 3, device=dev)
        r = L.TrRotArgs()
        r.gp, r.ld_gp, r.n_graphs, r.ns, r.sd, r.graph_emb = gpd.data_ptr(), 12, B, ns, sd, emb.data_ptr()
        for h in range(2):
            r.w1[h], r.b1[h], r.w2[h], r.b2[h] = (w[k][h].data_ptr() for k in ("w1", "b1", "w2", "b2"))
            r.sigma[h] = sig[h].data_ptr()
        r.so3_table, r.so3_n, r.so3_lo, r.so3_span = table.data_ptr(), SO3_N, float(np.float32(SO3_LO)), float(np.float32(SO3_HI - SO3_LO))
        r.out[0], r.out[1] = o_tr.data_ptr(), o_rot.data_ptr()
        L.check(lib.ddp_trrot_head(C.byref(r), K.stream()), "ddp_trrot_head")
        outs[name] = (o_tr.cpu().numpy(), o_rot.cpu().numpy())
    tr_ok, rot_ok = outs["ok"]
    tr_z, rot_z = outs["zero"]
    assert np.isfinite(tr_ok).all() and np.isfinite(rot_ok).all()
    assert np.isnan(tr_z[bad]).all(), "tr / |tr| with |tr| = 0 is NaN in the expression the kernel replaces"
    others = np.arange(B) != bad
    assert _same_bits(tr_z[others], tr_ok[others]) and _same_bits(rot_z, rot_ok)
    # ... and the finite rows are the expression in float64 (helpers.elementwise_excess(.., 1e-5) <= 1, the project's bound for
    # these heads in test_prologue_and_read_out_kernels_match_their_pytorch_definitions: 1e-5 |want| + 1e-6 max|want|)
    g64 = gp_ok.astype(np.float64)
    for h, (got, v) in enumerate(((tr_ok, g64[:, 0:3] + g64[:, 6:9]), (rot_ok, g64[:, 3:6] + g64[:, 9:12]))):
        nrm = np.linalg.norm(v, axis=1, keepdims=True)
        inp = np.concatenate([nrm, emb.cpu().numpy().astype(np.float64)], 1)
        hid = np.maximum(inp @ w["w1"][h].cpu().numpy().astype(np.float64).T + w["b1"][h].cpu().numpy().astype(np.float64), 0.0)
        mlp = hid @ w["w2"][h].cpu().numpy().astype(np.float64) + float(w["b2"][h][0])
        s = sig[h].cpu().numpy()
        norm = 1.0 / s.astype(np.float64) if h == 0 else (_so3_index32(s, np.float32(SO3_LO), np.float32(SO3_HI - SO3_LO), SO3_N) + 1.0)
        want = v / nrm * (mlp * norm)[:, None]
        _assert_within(got, want, 1e-5 * np.abs(want) + 1e-6 * np.abs(want).max(), f"trrot head {h}")


# ====================================================================================================== 4. small geometry kernels
def test_torsion_sh_degenerate_bonds_and_edges():
    """A bond vector of length 1e-20, one exactly 0, an edge harmonic [1, 0, 0, 0], a device-side edge count below the capacity
    (the tail of the output keeps its sentinel) and n_bonds = 0, against the dense form FullTensorProduct(sh, Y2(bond)) in
    float64 (oracle.thirdparty, as in test_edge_featurize_and_torsion_sh; its 1e-5).  Y2 is a homogeneous quadratic of the
    NORMALISED bond vector (F.normalize: v / max(|v|, 1e-12)): a zero bond gives a zero row, not -sqrt(3/2) n."""
    from oracle import thirdparty as tp
    L, lib, K = _api()
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    E, cap, T = 300, 333, 7
    vec = torch.randn(cap, 3, generator=g, dtype=torch.float64)
    vec[5] = 0.0                                                  # a zero-length edge: sh = [1, 0, 0, 0]
    sh = tp.spherical_harmonics("1x0e+1x1o", vec)
    bv = torch.randn(T, 3, generator=g, dtype=torch.float64)
    bv[1] = torch.tensor([1e-20, 0.0, 0.0], dtype=torch.float64)
    bv[2] = 0.0
    bv[3] = torch.tensor([0.0, -6e-21, 8e-21], dtype=torch.float64)
    bv = bv.float().double()
    boe = torch.randint(0, T, (cap,), generator=g)
    boe[:8] = torch.tensor([1, 2, 3, 0, 1, 2, 3, 4])              # every degenerate bond meets ordinary edges and the zero edge
    sh32 = sh.float()
    want = tp.FullTensorProduct("1x0e+1x1o", "2e")(sh32.double(), tp.spherical_harmonics("2e", bv)[boe])[:, :3].numpy()
    sh_d, bv_d, boe_d = sh32.to(dev).contiguous(), bv.float().to(dev).contiguous(), boe.int().to(dev)
    cnt = torch.tensor([E], dtype=torch.int32, device=dev)
    out = torch.full((cap, 4), float(SENTINEL), device=dev)
    L.check(lib.ddp_torsion_sh(K.ptr(sh_d), K.ptr(bv_d), K.ptr(boe_d), cap, K.ptr(cnt), K.ptr(out), None, 0, 0, None, None, 0, None,
                               K.stream()), "ddp_torsion_sh")
    got = out.cpu().numpy()
    assert (_bits(got[E:]) == _bits(np.full_like(got[E:], SENTINEL))).all(), "rows behind the device-side count were written"
    assert not got[:E, 0].any()
    _assert_within(got[:E, 1:], want[:E], np.full((E, 3), 1e-5), "torsion_sh")
    assert np.abs(want[[0, 1, 2, 4, 5, 6]]).max() < 1e-12 and np.abs(want[3]).max() > 0.01      # (the cases are what they claim)
    # n_bonds = 0 with a bond_attr array: nothing of it is written; n_edges = 0 as well: no launch, no error
    x = torch.randn(4, 8, device=dev)
    battr = torch.full((3, 8), float(SENTINEL), device=dev)
    idx = torch.zeros(3, dtype=torch.int32, device=dev)
    out.fill_(float(SENTINEL))
    L.check(lib.ddp_torsion_sh(K.ptr(sh_d), K.ptr(bv_d), K.ptr(boe_d), 8, None, K.ptr(out), K.ptr(x), 8, 8, K.ptr(idx), K.ptr(idx), 0,
                               K.ptr(battr), K.stream()), "ddp_torsion_sh")
    L.check(lib.ddp_torsion_sh(None, None, None, 0, None, None, K.ptr(x), 8, 8, K.ptr(idx), K.ptr(idx), 0, K.ptr(battr), K.stream()),
            "ddp_torsion_sh")
    assert (_bits(battr) == _bits(np.full((3, 8), SENTINEL))).all()
    _assert_within(out.cpu().numpy()[:8, 1:], want[:8], np.full((8, 3), 1e-5), "torsion_sh, 8 edges")


def _lattice(sizes, side, seed):
    """Distinct integer lattice points per graph (exact float32 distances, many exact ties)."""
    rng = np.random.default_rng(seed)
    pts, batch = [], []
    for i, n in enumerate(sizes):
        cells = rng.permutation(side ** 3)[:n]
        pts.append(np.stack([cells // (side * side), (cells // side) % side, cells % side], 1).astype(np.float32) + 10.0 * i)
        batch.append(np.full(n, i, np.int64))
    return torch.from_numpy(np.concatenate(pts)), torch.from_numpy(np.concatenate(batch))


@pytest.mark.parametrize("k", [1, 6, 26, 32])
def test_knn_with_exact_distance_ties(k):
    """Points on an integer lattice (every distance is tied many times over), several graphs of 1 - 64 points, k from 1 to the kernel's limit of 32 (>= the size of most of them):
    the pair list equals graph.knn_graph's dense formulation on the CPU - the definition, tie rule included."""
    from diffdock_pocket_amd import graph as G
    dev = _dev()
    for sizes, side in (([27, 27, 27], 3), ([40, 2, 1, 27, 9, 64], 4)):
        x, bx = _lattice(sizes, side, seed=k)
        lc, ld = G.DenseLayout.build(bx, len(sizes)), G.DenseLayout.build(bx.to(dev), len(sizes))
        want = G.knn_graph(x, k, lc)
        got = G.knn_graph(x.to(dev), k, ld).cpu()
        assert want.shape == got.shape and torch.equal(want, got), (k, sizes, want.shape, got.shape)


@pytest.mark.parametrize("rule", ["first_index", "nearest"])
def test_radius_searches_with_points_exactly_at_the_radius(rule):
    """Lattice points and r = 5: d^2 = 25 = r^2 exactly for the (3, 4, 0) and (5, 0, 0) offsets - the comparison is strict, they
    are no neighbours -, query points that coincide with x points (d = 0), a graph without queries and one without points, through
    ddp_radius_count + ddp_radius_fill (graph.radius / radius_graph) and ddp_radius_search_jobs, against the dense CPU form."""
    from diffdock_pocket_amd import graph as G
    L, lib, K = _api()
    dev = _dev()
    sizes_x, sizes_y = [60, 0, 30, 64], [20, 5, 0, 33]
    x, bx = _lattice(sizes_x, 7, seed=1)
    y, by = _lattice(sizes_y, 7, seed=2)
    y[:10] = x[:10]                                               # coincident query and x points
    B = 4
    d2 = ((y[by == 0][:, None, :] - x[bx == 0][None, :, :]) ** 2).sum(-1)
    assert int((d2 == 25.0).sum()) > 0 and int((d2 == 0.0).sum()) >= 10
    lx, ly = G.DenseLayout.build(bx, B), G.DenseLayout.build(by, B)
    lxd, lyd = G.DenseLayout.build(bx.to(dev), B), G.DenseLayout.build(by.to(dev), B)
    xd, yd = x.to(dev), y.to(dev)
    for cap in (10000, 6):
        want = G.radius(x, y, 5.0, lx, ly, max_num_neighbors=cap, truncation=rule)
        got = G.radius(xd, yd, 5.0, lxd, lyd, max_num_neighbors=cap, truncation=rule).cpu()
        assert want.shape == got.shape and torch.equal(want, got), (cap, rule, want.shape, got.shape)
        want_g = G.radius_graph(x, 5.0, lx, max_num_neighbors=cap, truncation=rule)
        got_g = G.radius_graph(xd, 5.0, lxd, max_num_neighbors=cap, truncation=rule).cpu()
        assert torch.equal(want_g, got_g), (cap, rule)
        # the same two searches as jobs of one launch
        G._ptr(lxd), G._ptr(lyd)
        ny, nx = y.shape[0], x.shape[0]
        flags = 2 if rule == "nearest" else 0
        i32e = lambda n: torch.full((n,), -1, dtype=torch.int32, device=dev)      # noqa: E731
        room, room_g = want.shape[1] + 5, want_g.shape[1] + 5
        oq, ox, tot, gq, gx, gtot = i32e(room), i32e(room), i32e(1), i32e(room_g), i32e(room_g), i32e(1)
        jobs = [K.radius_job(xd, lxd._ptr32, yd, G._batch32(lyd, ny), 5.0, cap, flags, i32e(ny), i32e(ny + 1), total=tot, out_query=oq,
                             out_x=ox, capacity=room),
                K.radius_job(xd, lxd._ptr32, xd, G._batch32(lxd, nx), 5.0, cap + 1, flags | 1, i32e(nx), i32e(nx + 1), total=gtot,
                             out_query=gq, out_x=gx, capacity=room_g)]
        K.radius_search_jobs(jobs)
        torch.cuda.synchronize()
        E, Eg = want.shape[1], want_g.shape[1]
        assert int(tot.item()) == E and int(gtot.item()) == Eg
        assert torch.equal(oq[:E].cpu().long(), want[0]) and torch.equal(ox[:E].cpu().long(), want[1])
        assert torch.equal(gx[:Eg].cpu().long(), want_g[0]) and torch.equal(gq[:Eg].cpu().long(), want_g[1])
        assert bool((oq[E:] == -1).all()) and bool((gq[Eg:] == -1).all())


def test_pose_update_at_the_edges_of_its_branches():
    """Rotation vectors of norm pi, 2e-6 and 5e-7 (both sides of the small-angle branch at 1e-6), torsions of exactly +pi / -pi,
    T = 0 with non-null arrays, one sample - against the batched float64 modify_conformer (tests/test_sampler_cpu.py pins it to the
    reference's functions) with the project's bound of test_pose_update_kernel_matches_modify_conformer: 2e-5 max|want|."""
    from diffdock_pocket_amd import sampler as S
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    L, lib, K = _api()
    dev = _dev()
    g = make_3dpf_complex(seed=0, flexible_sidechains=False)
    em = g["ligand"].edge_mask.bool()
    bonds = g["ligand", "ligand"].edge_index.t()[em].clone()
    mr = g["ligand"].mask_rotate
    mask = torch.as_tensor(np.asarray(mr if isinstance(mr, np.ndarray) else mr[0])).bool()
    T, n = bonds.shape[0], g["ligand"].pos.shape[0]
    assert T > 0
    gen = torch.Generator().manual_seed(6)
    N = 6
    pos = g["ligand"].pos.unsqueeze(0).repeat(N, 1, 1) + torch.randn(N, 1, 3, generator=gen) * 3
    tr = torch.randn(N, 3, generator=gen) * 0.5
    axis = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    rot = axis * torch.tensor([math.pi, 2e-6, 5e-7, math.pi, 0.7, 2e-6]).unsqueeze(1)
    tor = torch.randn(N, T, generator=gen) * 0.6
    tor[0], tor[1], tor[2, ::2], tor[2, 1::2], tor[3, 0] = math.pi, -math.pi, math.pi, -math.pi, math.pi
    pos, tr, rot, tor = pos.float(), tr.float(), rot.float(), tor.float()
    bonds_d, mask_d = bonds.to(torch.int32).to(dev), mask.to(torch.uint8).to(dev)

    def check(sel, with_tor, what):
        p, t_, r_, o_ = pos[sel], tr[sel], rot[sel], tor[sel]
        want = S.modify_conformer(p.double(), t_.double(), r_.double(), o_.double() if with_tor else None, bonds, mask).numpy()
        got = S.modify_conformer_hip(p.to(dev), t_.to(dev), r_.to(dev), o_.to(dev) if with_tor else None, bonds_d if with_tor else None,
                                     mask_d if with_tor else None).cpu().numpy()
        _assert_within(got, want, np.full(want.shape, 2e-5 * float(np.abs(want).max())), what)
        return want

    check(slice(0, N), True, "pose_update, 6 samples")
    check(slice(0, N), False, "pose_update, rigid")
    for s in range(3):
        check(slice(s, s + 1), True, f"pose_update, one sample ({s})")
    # T = 0 with non-null torsion arrays: the rigid move
    want = S.modify_conformer(pos.double(), tr.double(), rot.double(), None, bonds, mask).numpy()
    pd, td, rd, od, out = pos.to(dev).contiguous(), tr.to(dev), rot.to(dev), tor.to(dev).contiguous(), torch.empty(N, n, 3, device=dev)
    L.check(lib.ddp_pose_update(pd.data_ptr(), N, n, td.data_ptr(), rd.data_ptr(), od.data_ptr(), 0, bonds_d.data_ptr(), mask_d.data_ptr(),
                                out.data_ptr(), torch._C._cuda_getCurrentRawStream(pd.device.index)), "ddp_pose_update")
    _assert_within(out.cpu().numpy(), want, np.full(want.shape, 2e-5 * float(np.abs(want).max())), "pose_update, T = 0")
