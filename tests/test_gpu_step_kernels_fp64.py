"""The kernels that open and close every denoising step, each against the definition in include/ddp_hip.h evaluated in float64 on
the CPU, element by element: ddp_edge_featurize (scalar and matrix-core form) / ddp_edge_featurize_jobs, ddp_step_prologue,
ddp_trrot_head / ddp_tor_head, ddp_sidechain_update, ddp_sde_update.  In the manner of tests/test_gpu_kernels_fp64.py: seeded numpy
inputs, calls through the C ABI, no kernel of the library is the reference for another (bitwise comparisons of two forms or two
launches are extra assertions), memory a kernel must not write holds a sentinel that is compared bit for bit.

Bounds are derived in the docstrings from the inputs (u = 2^-24; a K-term fp32 sum started from a given value is held to
(K + 2) u sum |a_k| |w_k|).  The only measured numbers are the device transcendentals - expf, powf, sinf / cosf, tanhf -, each
against a yardstick: torch-ROCm's float32 function on the grid of arguments the tests form, compared with numpy float64; the kernel
is allowed twice the yardstick (each yardstick is printed when it is taken).  The score-norm lookups behind log10f / logf are pinned by
tests/test_gpu_kernels_fp64.py; here the tables are all ones, so that the logarithm cannot move a result.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import SENTINEL, _assert_within, _bits, _up

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
TINY = 2.0 ** -126                     # smallest normal float32: what a flushed or subnormal Gaussian can be off by
ISENT = np.int32(-77777)
F64 = np.float64


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda")


def _api():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import launch as K
    return L, L.load(), K


def _sent(shape, dev):
    return torch.full(shape, float(SENTINEL), device=dev)


def _is_sentinel(a):
    return bool((_bits(a) == _bits(np.full(1, SENTINEL))[0]).all())


def _padded(a, pad):
    """`pad` NaN columns behind the used ones: a kernel that reads one shows it."""
    return np.concatenate([a, np.full((a.shape[0], pad), np.nan, np.float32)], 1) if pad else a


_YARD = {}


def _yardstick(name, dev, fn, ref, args, relative, floor=0.0):
    """max |torch-ROCm float32 fn - float64 ref| over `args` (relative to |ref| where asked, over the results >= floor), computed
    once per name.  Held to 2^-22 (relative) / 2^-22 (absolute, values <= 1): beyond that the grid has to shrink, not the
    allowance to grow."""
    if name not in _YARD:
        got = fn(*[_up(a, dev) for a in args]).cpu().numpy().astype(F64)
        want = ref(*[a.astype(F64) for a in args])
        err = np.abs(got - want)
        if relative:
            keep = np.abs(want) >= floor
            err = err[keep] / np.abs(want[keep])
        worst = float(err.max()) if err.size else 0.0
        assert worst <= 2.0 ** -22, f"torch-ROCm {name} is off by {worst:.3e} > 2^-22 on the tests' grid: no yardstick for the kernel"
        print(f"[fp64] {name} yardstick (torch-ROCm float32 against float64, {'relative' if relative else 'absolute'}): {worst:.3e}")
        _YARD[name] = worst
    return _YARD[name]


# ====================================================================================================== 1. edge featurisation
# Every featurisation test draws its edges from ONE fixed pair of point sets, so that every distance - and with the fixed list of
# k_rbf below every Gaussian argument - a test can form is known beforehand: the expf yardstick is taken on that grid, with d
# evaluated by numpy in float32.  The kernel's own d may differ from numpy's by an ulp (another summation order, another square
# root), so its arguments are that grid or its nearest neighbours; the allowance of twice the yardstick is meant to cover that.
_FEAT_KS = (2, 8, 10, 16, 24, 32, 33, 40, 48, 50, 56, 64, 65, 100, 256)
_N_PTS = 37


def _points():
    rng = np.random.default_rng(12345)
    a = (rng.standard_normal((_N_PTS, 3)) * 2.5).astype(np.float32)
    b = (rng.standard_normal((_N_PTS, 3)) * 2.5).astype(np.float32)
    b[0] = a[0]                                   # pair (0, 0): an edge of exactly zero length
    b[1] = np.float32([1500.0, -900.0, 400.0])    # every pair (., 1): so long that every Gaussian underflows
    return a, b


_POS_A, _POS_B = _points()


def _smearing(k):
    """GaussianSmearing(0, 5, k) (models/score_model.py:661-671)."""
    off = np.linspace(0.0, 5.0, k).astype(np.float32)
    return off, np.float32(-0.5 / float(off[1] - off[0]) ** 2)


def _gauss_args32(d32, off, coeff):
    t = (d32[:, None] - off[None, :]).astype(np.float32)
    return (coeff * (t * t).astype(np.float32)).astype(np.float32)


def _exp_yardstick(dev):
    """Relative error of torch.exp (ROCm, float32) over coeff_k (d - offset_k[j])^2 in float32 for all 37 x 37 distances of the
    fixed point sets and every k_rbf of _FEAT_KS (results below the smallest normal float32 are left out: the bound carries an
    absolute 2^-126 for them)."""
    v = (_POS_B[None, :, :] - _POS_A[:, None, :]).reshape(-1, 3)
    d32 = np.sqrt((v * v).sum(1, dtype=np.float32)).astype(np.float32)
    args = np.concatenate([_gauss_args32(d32, *_smearing(k)).ravel() for k in _FEAT_KS])
    return _yardstick("expf", dev, torch.exp, np.exp, [args], True, TINY)


class _Case:
    pass


def _feat_case(seed, dev, E, ns, k, n_pre2=0, cap=None, count=None, idx="random", special=True, dead_last_k=False):
    """One featurisation problem.  E: live edges if no device-side count is given; cap: n_edges handed over (the arrays' capacity,
    default E); count: value of *n_edges_dev (None: no count) - the live edges are min(cap, count).  ld_pre = ns + 3, ld_pre2 =
    ns + 5, the padding NaN.  idx: random (11 rows: repeats) | last (the second half of the edges all read the LAST pre row).
    special: edge 1 has zero length, edge 2 is 1.8e3 long (where there are that many edges).  dead_last_k: row k - 1 of w1d is
    zero (that Gaussian multiplies 0: the problem is the one with k - 1 Gaussians)."""
    assert k in _FEAT_KS
    rng = np.random.default_rng(seed)
    c = _Case()
    cap = E if cap is None else cap
    c.cap, c.count, c.ns, c.k, c.n_pre2 = cap, count, ns, k, n_pre2
    c.n = cap if count is None else max(0, min(cap, count))
    c.ia = rng.integers(2, _N_PTS, cap).astype(np.int32)
    c.ib = rng.integers(2, _N_PTS, cap).astype(np.int32)
    if special and cap > 1:
        c.ia[1] = c.ib[1] = 0
    if special and cap > 2:
        c.ib[2] = 1
    c.off, c.coeff = _smearing(k)
    n_rows = 11
    c.pre = rng.standard_normal((n_rows, ns)).astype(np.float32)
    c.pre_idx = rng.integers(0, n_rows, cap).astype(np.int32)
    if idx == "last":
        c.pre_idx[cap // 2:] = n_rows - 1
    c.pre2 = (rng.standard_normal((n_pre2, ns)) * 0.7).astype(np.float32) if n_pre2 else None
    c.w1 = (rng.standard_normal((k, ns)) * 0.5).astype(np.float32)
    if dead_last_k:
        c.w1[k - 1] = 0.0
    c.w2 = (rng.standard_normal((ns, ns)) / math.sqrt(ns)).astype(np.float32)
    c.b2 = rng.standard_normal(ns).astype(np.float32)
    w1d, w2p, b2p = np.zeros((k, 64), np.float32), np.zeros((64, 64), np.float32), np.zeros(64, np.float32)
    w1d[:, :ns], w2p[:ns, :ns], b2p[:ns] = c.w1, c.w2, c.b2
    c.d = dict(pos_a=_up(_POS_A, dev), pos_b=_up(_POS_B, dev), ia=_up(c.ia, dev), ib=_up(c.ib, dev), off=_up(c.off, dev),
               pre=_up(_padded(c.pre, 3), dev), pre_idx=_up(c.pre_idx, dev), w1d=_up(w1d, dev), w2=_up(w2p, dev), b2=_up(b2p, dev),
               pre2=_up(_padded(c.pre2, 5), dev) if n_pre2 else None,
               cnt=torch.tensor([count], dtype=torch.int32, device=dev) if count is not None else None,
               out=_sent((max(cap, 1), ns), dev), sh=_sent((max(cap, 1), 4), dev))
    return c


def _feat_job(c):
    L, lib, K = _api()
    d, j = c.d, L.FeaturizeJob()
    j.pos_a, j.ia, j.pos_b, j.ib, j.n_edges, j.n_edges_dev = K._p(d["pos_a"]), K._p(d["ia"]), K._p(d["pos_b"]), K._p(d["ib"]), c.cap, K._p(d["cnt"])
    j.offset, j.k_rbf, j.coeff = K._p(d["off"]), c.k, float(c.coeff)
    j.pre, j.pre_idx, j.ld_pre = K._p(d["pre"]), K._p(d["pre_idx"]), c.ns + 3
    j.pre2, j.n_pre2, j.ld_pre2 = K._p(d["pre2"]), c.n_pre2, c.ns + 5
    j.w1d, j.w2, j.b2, j.ns, j.out, j.sh = K._p(d["w1d"]), K._p(d["w2"]), K._p(d["b2"]), c.ns, K._p(d["out"]), K._p(d["sh"])
    return j


def _feat_single(c, **over):
    """Through ddp_edge_featurize; `over` replaces arguments (the refusal tests)."""
    L, lib, K = _api()
    d = c.d
    a = dict(k=c.k, ns=c.ns, pre2=d["pre2"], n_pre2=c.n_pre2)
    a.update(over)
    return lib.ddp_edge_featurize(K.ptr(d["pos_a"]), K.ptr(d["ia"]), K.ptr(d["pos_b"]), K.ptr(d["ib"]), c.cap, K.ptr(d["cnt"]),
                                  K.ptr(d["off"]), a["k"], C.c_float(float(c.coeff)), K.ptr(d["pre"]), K.ptr(d["pre_idx"]), c.ns + 3,
                                  K.ptr(a["pre2"]), a["n_pre2"], c.ns + 5, K.ptr(d["w1d"]), K.ptr(d["w2"]), K.ptr(d["b2"]), a["ns"],
                                  K.ptr(d["out"]), K.ptr(d["sh"]), K.stream())


def _feat_jobs(cases):
    L, lib, K = _api()
    arr = (L.FeaturizeJob * max(len(cases), 1))(*[_feat_job(c) for c in cases])
    return lib.ddp_edge_featurize_jobs(arr, len(cases), K.stream())


def _feat_reset(c):
    c.d["out"].fill_(float(SENTINEL))
    c.d["sh"].fill_(float(SENTINEL))


def _feat_ref(c, eps_exp):
    """The header's definition in float64 and the forward bound, for the live edges.  vec = pos_b[ib] - pos_a[ia] is ONE float32
    subtraction per component (the kernel's own; the definition starts from it).  With u = 2^-24:
      d      three squares, two adds, a square root:                              |dd| <= 3 u d
      t_k    = d - offset_k, one subtraction:                                     |dt| <= dd + u |t_k|
      a_k    = coeff t_k^2, two products:                                         |da| <= |coeff| (2 |t_k| dt + dt^2) + 3 u |a_k|
      rbf_k  = exp(a_k), device expf with relative error eps_exp (2 x the yardstick):
                                                                                  |dr| <= (e^(a + da) - e^a) + eps_exp e^(a + da) + 2^-126
      hid_j  = pre + pre2 + sum_k rbf_k w1d[k, j], a k_rbf-term sum from (pre + pre2):
                                                                                  |dh| <= (k_rbf + 2) u (|pre| + |pre2| + sum rbf |w|) + sum dr |w|
      out_c  = b2 + sum_j relu(hid_j) w2[j, c] (relu is 1-Lipschitz; the padded terms j >= ns add exact zeros):
                                                                                  |do| <= (ns + 2) u (|b2| + sum (relu + dh) |w2|) + sum dh |w2|
      sh     = [1, sqrt(3) vec / max(d, 1e-12)]: the constant, d (3 u), the division, the product: 7 u |sh|; the 1 exact."""
    n, ns, k = c.n, c.ns, c.k
    v = (_POS_B[c.ib[:n]] - _POS_A[c.ia[:n]]).astype(F64)
    d = np.sqrt((v * v).sum(1))
    off, co = c.off.astype(F64), float(c.coeff)
    t = d[:, None] - off[None, :]
    dt = 3 * U24 * d[:, None] + U24 * np.abs(t)
    a = co * t * t
    da = abs(co) * (2 * np.abs(t) * dt + dt * dt) + 3 * U24 * np.abs(a)
    rbf, hi = np.exp(a), np.exp(a + da)
    dr = (hi - rbf) + eps_exp * hi + TINY
    w1, w2 = c.w1.astype(F64), c.w2.astype(F64)
    start = c.pre.astype(F64)[c.pre_idx[:n]]
    mag = np.abs(start)
    m2 = min(c.n_pre2, n)
    if m2:
        start[:m2] += c.pre2.astype(F64)[:m2]
        mag[:m2] += np.abs(c.pre2.astype(F64)[:m2])
    hid = start + rbf @ w1
    dh = (k + 2) * U24 * (mag + rbf @ np.abs(w1)) + dr @ np.abs(w1)
    r = np.maximum(hid, 0.0)
    out = c.b2.astype(F64) + r @ w2
    tol = (ns + 2) * U24 * (np.abs(c.b2.astype(F64)) + (r + dh) @ np.abs(w2)) + dh @ np.abs(w2)
    sh = np.concatenate([np.ones((n, 1)), math.sqrt(3.0) * v / np.maximum(d, 1e-12)[:, None]], 1)
    return out, tol, sh, 7 * U24 * np.abs(sh) * np.float64([0, 1, 1, 1]), d


def _feat_check(c, dev, what, ref=None):
    """out / sh of the live edges within the bound of _feat_ref; rows behind the count keep the sentinel; the zero-length edge gives
    sh = [1, 0, 0, 0] bit for bit and the long one a finite row."""
    ref = ref or _feat_ref(c, 2.0 * _exp_yardstick(dev))
    out, tol, sh, tol_sh, d = ref
    n = c.n
    got, got_sh = c.d["out"].cpu().numpy(), c.d["sh"].cpu().numpy()
    assert _is_sentinel(got[n:]) and _is_sentinel(got_sh[n:]), f"{what}: a row behind the edge count was written"
    if n:
        _assert_within(got[:n], out, tol, what)
        _assert_within(got_sh[:n], sh, tol_sh, what + " sh")
        zero = d == 0.0
        assert np.array_equal(_bits(got_sh[:n][zero]), _bits(np.tile(np.float32([1, 0, 0, 0]), (int(zero.sum()), 1)))), f"{what}: sh of a zero-length edge"
    return got.copy(), got_sh.copy()


def _feat_both_entries(c, dev, what):
    """A matrix-core problem through ddp_edge_featurize and through ddp_edge_featurize_jobs: both within the bound, and the same bits."""
    ref = _feat_ref(c, 2.0 * _exp_yardstick(dev))
    assert _feat_single(c) == 0, what
    a = _feat_check(c, dev, what, ref)
    _feat_reset(c)
    assert _feat_jobs([c]) == 0, what
    b = _feat_check(c, dev, what + " (jobs)", ref)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), f"{what}: the two entry points differ"


def test_featurize_special_edges_are_what_they_claim():
    """Inputs only, no kernel runs: pair (0, 0) has d = 0 exactly, and a pair (., 1) is about 1.8e3 long.  Every Gaussian of such an
    edge has the argument coeff_k (d - offset)^2 <= coeff_k (d - 5)^2 (offsets lie in [0, 5]); that is < -1e4 for every k_rbf the
    tests use - k_rbf = 2 has the weakest coefficient, -0.02, and gives about -6.4e4 -, so exp underflows to 0 in float32 and in
    float64 (which underflows below -745)."""
    c = _feat_case(0, torch.device("cpu"), 8, 4, 2)
    d = _feat_ref(c, 0.0)[4]
    assert d[1] == 0.0 and d[2] > 1.7e3
    for k in _FEAT_KS:
        assert float(_smearing(k)[1]) * (d[2] - 5.0) ** 2 < -1e4, k


@pytest.mark.parametrize("ns", [1, 16, 31, 32, 33, 60, 64])
def test_featurize_mfma_rows_and_columns_on_the_tile_edges(ns):
    """k_rbf = 32, E in {1, 31, 32, 33, 127, 128, 129, 257} (the 32-edge wave tile, the 128-edge workgroup) x ns around the two
    32-column halves (r < ns, 32 + r < ns), a second table on the first 5 edges."""
    dev = _dev()
    for E in (1, 31, 32, 33, 127, 128, 129, 257):
        c = _feat_case(100 * ns + E, dev, E, ns, 32, n_pre2=min(5, E))
        _feat_both_entries(c, dev, f"featurize mfma E={E} ns={ns}")


@pytest.mark.parametrize("k", [8, 16, 56, 64])
def test_featurize_mfma_k_rbf(k):
    """k_rbf = 8, 16 (< 32), 56, 64 at the ragged shape E = 129, ns = 33."""
    dev = _dev()
    _feat_both_entries(_feat_case(k, dev, 129, 33, k, n_pre2=7), dev, f"featurize mfma k_rbf={k}")


@pytest.mark.parametrize("form_k", [32, 50])
def test_featurize_second_table_and_row_index(form_k):
    """n_pre2 in {0, 1, 5, 32, 33, E, E + 7} (inside a 32-edge tile, on its edge, beyond the edge list) with ld_pre, ld_pre2 > ns
    and NaN padding of their own, ns = 60 (both column halves add pre2); a pre_idx full of repeats, and one whose repeated row is
    the table's last.  form_k = 32: matrix-core form, 50: scalar form."""
    dev = _dev()
    E = 97
    for i, n_pre2 in enumerate((0, 1, 5, 32, 33, E, E + 7)):
        c = _feat_case(7 * form_k + i, dev, E, 60, form_k, n_pre2=n_pre2, idx="last" if i & 1 else "random")
        if form_k == 32:
            _feat_both_entries(c, dev, f"featurize mfma n_pre2={n_pre2}")
        else:
            assert _feat_single(c) == 0
            _feat_check(c, dev, f"featurize scalar n_pre2={n_pre2}")


@pytest.mark.parametrize("form_k", [32, 10])
def test_featurize_device_side_counts(form_k):
    """*n_edges_dev equal to the capacity, below it (inside a tile), 0 and above it (clamped to the capacity): rows of out and sh
    behind the count keep the sentinel."""
    dev = _dev()
    cap = 200
    for count in (cap, 77, 0, cap + 50):
        c = _feat_case(form_k + count, dev, cap, 33, form_k, n_pre2=90, cap=cap, count=count)
        assert c.n == min(cap, count)
        if form_k == 32:
            _feat_both_entries(c, dev, f"featurize mfma count={count}")
        else:
            assert _feat_single(c) == 0
            _feat_check(c, dev, f"featurize scalar count={count}")


@pytest.mark.parametrize("k", [2, 10, 50, 65, 100, 256])
def test_featurize_scalar_form(k):
    """The one-thread-per-edge form (any k_rbf that is not a multiple of 8 in [8, 64]): E in {1, 63, 64, 65, 255, 256, 257} (the
    64-edge wave transpose, the 256-edge workgroup) x ns in {1, 33, 64}."""
    dev = _dev()
    for E in (1, 63, 64, 65, 255, 256, 257):
        for ns in (1, 33, 64):
            c = _feat_case(1000 * k + 3 * E + ns, dev, E, ns, k, n_pre2=min(3, E))
            assert _feat_single(c) == 0, (k, E, ns)
            _feat_check(c, dev, f"featurize scalar k_rbf={k} E={E} ns={ns}")


def test_featurize_the_two_forms_on_one_problem():
    """The scalar form cannot be reached with k_rbf = 32; with k_rbf = 33 and a zero last row of w1d it computes the same 32-term
    problem.  Both forms are held to the COMMON float64 definition (whose value the dead Gaussian does not change), never to each other."""
    dev = _dev()
    a = _feat_case(5, dev, 257, 60, 33, n_pre2=40, dead_last_k=True)
    b = _feat_case(5, dev, 257, 60, 32, n_pre2=40)
    b.ia, b.ib, b.pre, b.pre_idx, b.pre2, b.w1, b.w2, b.b2 = a.ia, a.ib, a.pre, a.pre_idx, a.pre2, a.w1[:32].copy(), a.w2, a.b2
    b.off, b.coeff = a.off[:32].copy(), a.coeff               # the 33-point grid's first 32 offsets and ITS coefficient
    w1d = np.zeros((32, 64), np.float32)
    w1d[:, :60] = b.w1
    w2p, b2p = np.zeros((64, 64), np.float32), np.zeros(64, np.float32)
    w2p[:60, :60], b2p[:60] = b.w2, b.b2
    b.d.update(ia=_up(b.ia, dev), ib=_up(b.ib, dev), pre=_up(_padded(b.pre, 3), dev), pre_idx=_up(b.pre_idx, dev),
               pre2=_up(_padded(b.pre2, 5), dev), w1d=_up(w1d, dev), w2=_up(w2p, dev), b2=_up(b2p, dev), off=_up(b.off, dev))
    eps = 2.0 * _exp_yardstick(dev)
    ref_a, ref_b = _feat_ref(a, eps), _feat_ref(b, eps)
    assert np.array_equal(ref_a[0], ref_b[0]) or np.abs(ref_a[0] - ref_b[0]).max() < 1e-13
    assert _feat_single(a) == 0 and _feat_single(b) == 0
    _feat_check(a, dev, "featurize scalar, 32 live Gaussians", ref_a)
    _feat_check(b, dev, "featurize mfma, the same 32 Gaussians", ref_b)


def test_featurize_mfma_second_trip_of_the_stride_loop():
    """E = 1024 x 128 + 33, ns = 16, k_rbf = 8: the smallest size at which a workgroup of the matrix-core form walks a second tile."""
    dev = _dev()
    c = _feat_case(1, dev, 1024 * 128 + 33, 16, 8, n_pre2=33)
    assert _feat_single(c) == 0
    _feat_check(c, dev, "featurize mfma, second trip")


def test_featurize_scalar_second_trip_of_the_stride_loop():
    """E = 2048 x 256 + 65, ns = 3, k_rbf = 10: the same for the scalar form's 2048-workgroup cap."""
    dev = _dev()
    c = _feat_case(2, dev, 2048 * 256 + 65, 3, 10, n_pre2=65)
    assert _feat_single(c) == 0
    _feat_check(c, dev, "featurize scalar, second trip")


def test_featurize_eight_jobs_in_one_launch():
    """Eight jobs with different k_rbf (the smallest not first: the LDS carve-up is sized by the launch's largest), different ns
    and sizes, an empty job in the middle, one with a device-side count: every job within its fp64 bound, and bit for bit what its
    own launch writes."""
    dev = _dev()
    spec = [(300, 60, 32, {}), (129, 16, 8, {}), (1, 64, 64, {}), (0, 24, 16, {}), (700, 33, 56, dict(cap=700, count=333)),
            (257, 1, 24, {}), (33, 31, 40, {}), (128, 32, 48, {})]
    cases = [_feat_case(50 + i, dev, E, ns, k, n_pre2=min(E, 9 * i), **kw) for i, (E, ns, k, kw) in enumerate(spec)]
    eps = 2.0 * _exp_yardstick(dev)
    refs = [_feat_ref(c, eps) for c in cases]
    single = []
    for i, c in enumerate(cases):
        assert _feat_single(c) == 0
        single.append(_feat_check(c, dev, f"featurize job {i} alone", refs[i]))
        _feat_reset(c)
    assert _feat_jobs(cases) == 0
    for i, c in enumerate(cases):
        got = _feat_check(c, dev, f"featurize job {i} of 8", refs[i])
        assert np.array_equal(_bits(got[0]), _bits(single[i][0])) and np.array_equal(_bits(got[1]), _bits(single[i][1])), f"job {i}"


def test_featurize_refuses_what_it_cannot_run():
    """Nine jobs; k_rbf = 12 in a job (the same problem runs through ddp_edge_featurize); ns = 65, k_rbf = 1 and 257, n_pre2 > 0
    with pre2 NULL through both entry points: an error code, nothing written."""
    dev = _dev()
    c = _feat_case(3, dev, 40, 16, 16, n_pre2=5)
    assert _feat_jobs([c] * 9) != 0
    assert _feat_single(c, ns=65) != 0 and _feat_single(c, k=1) != 0 and _feat_single(c, k=257) != 0
    assert _feat_single(c, pre2=None, n_pre2=5) != 0
    L, lib, K = _api()
    for field, value in (("ns", 65), ("k_rbf", 12), ("k_rbf", 1), ("k_rbf", 257), ("pre2", 0)):
        j = _feat_job(c)
        setattr(j, field, value)
        assert lib.ddp_edge_featurize_jobs((L.FeaturizeJob * 1)(j), 1, K.stream()) != 0, field
    torch.cuda.synchronize()
    assert _is_sentinel(c.d["out"]) and _is_sentinel(c.d["sh"])
    # ... and k_rbf = 12 is a problem ddp_edge_featurize takes (the scalar form): the first 12 offsets of the 16-point grid
    assert _feat_single(c, k=12) == 0
    c.k, c.off, c.w1 = 12, c.off[:12], c.w1[:12]
    ref = _feat_ref(c, 2.0 * _exp_yardstick(dev))
    _feat_check(c, dev, "featurize k_rbf=12 through ddp_edge_featurize", ref)


# ====================================================================================================== 2. ddp_step_prologue
_T_GRID = 4096                                   # diffusion times are multiples of 1 / 4096, as in test_gpu_kernels_fp64.py
_SIG_RANGES = ((0.1, 19.0), (0.03, 1.55), (0.0314, 3.14), (0.0314, 3.14))
_EMB_SCALE = 1000.0
_PROLOGUE_SDS = (2, 32, 33, 64)


def _freq(sd):
    half = sd // 2
    if half == 1:
        return np.ones(1, np.float32)
    return np.exp(np.arange(half, dtype=np.float32) * np.float32(-(math.log(10000.0) / (half - 1)))).astype(np.float32)


def _emb_args(t32, freq32):
    st = (np.float32(_EMB_SCALE) * t32.astype(np.float32)).astype(np.float32)
    return (st[:, None] * freq32[None, :]).astype(np.float32)


def _grid_t():
    return (np.arange(_T_GRID + 1, dtype=F64) / _T_GRID).astype(np.float32)


def _pow_yardstick(dev):
    """Relative error of torch.pow (ROCm, float32) over sig_min^(1 - t) and sig_max^t, t = i / 4096, for the four sigma ranges."""
    t = _grid_t()
    base = np.concatenate([np.full(t.shape, v, np.float32) for lo, hi in _SIG_RANGES for v in (lo, hi)])
    expo = np.concatenate([e for _ in _SIG_RANGES for e in ((np.float32(1) - t).astype(np.float32), t)])
    return _yardstick("powf", dev, torch.pow, np.power, [base, expo], True)


def _sincos_yardstick(dev):
    """Absolute error of torch.sin / torch.cos (ROCm, float32) over (1000 t) freq[s] in float32, t = i / 4096, the frequencies
    of sd = 2, 32 / 33 and 64."""
    args = np.concatenate([_emb_args(_grid_t(), _freq(sd)).ravel() for sd in (2, 32, 64)])
    return max(_yardstick("sinf", dev, torch.sin, np.sin, [args], False), _yardstick("cosf", dev, torch.cos, np.cos, [args], False))


def _prologue_case(seed, dev, sizes, n_bonds, n_copy, sd, t_stride, modes, with_emb=True):
    """sizes: atoms per graph; n_bonds / n_copy: the two bond jobs' and the two copies' lengths; modes[k]: c (sigma computed) |
    i (sigma an input: sig_max = 0) | n (NULL).  Every output buffer is longer than what the kernel may write, sentinel behind.
    Both bond jobs' first bond joins two atoms at 3e38 and 2.5e38: (u + v) / 2 overflows in float32, as the definition says."""
    L, lib, K = _api()
    rng = np.random.default_rng(seed)
    c = _Case()
    B = len(sizes)
    c.B, c.sizes, c.sd, c.modes, c.n_bonds, c.n_copy, c.keep = B, sizes, sd, modes, n_bonds, n_copy, []

    def up(a):
        t = _up(a, dev)
        c.keep.append(t)
        return t

    a = L.PrologueArgs()
    a.n_graphs = B
    nt = max(B, 1)
    tb = (rng.integers(0, _T_GRID + 1, (nt, 4)) / _T_GRID).astype(np.float32)
    if t_stride == 0:
        tb[:] = tb[0]
    c.t = tb[:B]
    d_tb = up(tb)                                            # stride 4: the four components' times interleaved in ONE buffer
    d_t1 = [up(tb[:, k].copy()) for k in range(4)]
    c.sig_in = (rng.random((4, nt)) + 0.25).astype(np.float32)
    c.d_sig = []
    for k in range(4):
        a.t[k] = d_tb.data_ptr() + 4 * k if t_stride == 4 else d_t1[k].data_ptr()
        a.t_stride[k] = t_stride
        a.sig_min[k], a.sig_max[k] = _SIG_RANGES[k][0], (_SIG_RANGES[k][1] if modes[k] == "c" else 0.0)
        buf = np.full(nt + 2, SENTINEL, np.float32)
        if modes[k] == "i":
            buf[:B] = c.sig_in[k, :B]
        c.d_sig.append(up(buf))
        a.sigma[k] = c.d_sig[k].data_ptr() if modes[k] != "n" else 0
    c.d_cut = _sent((nt + 2,), dev)
    c.cut_mul, c.cut_add = np.float32(3.0), np.float32(20.0)
    if modes[0] != "n":
        a.cut, a.cut_mul, a.cut_add = c.d_cut.data_ptr(), 3.0, 20.0
    c.freq = _freq(sd)
    c.d_emb = _sent((nt + 1, sd), dev)
    c.with_emb = with_emb
    if with_emb:
        a.graph_emb, a.sd, a.emb_scale, a.freq = c.d_emb.data_ptr(), sd, _EMB_SCALE, up(c.freq).data_ptr()
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    c.ptr = ptr
    c.lig = (rng.standard_normal((max(int(ptr[-1]), 1), 3)) * 5 + rng.standard_normal(3) * 20).astype(np.float32)
    c.d_cen = _sent((nt + 1, 3), dev)
    a.lig_pos, a.graph_ptr, a.center = up(c.lig).data_ptr(), up(ptr).data_ptr(), c.d_cen.data_ptr()
    c.bonds = []
    for h in range(2):
        n = n_bonds[h]
        pos = (rng.standard_normal((50, 3)) * 6).astype(np.float32)
        pos[0], pos[1] = np.float32(3e38), np.float32(2.5e38)
        b0, b1 = rng.integers(2, 50, max(n, 1)).astype(np.int32), rng.integers(2, 50, max(n, 1)).astype(np.int32)
        b0[0], b1[0] = 0, 1
        mid, vec = _sent((n + 3, 3), dev), _sent((n + 3, 3), dev)
        c.bonds.append((pos, b0[:n], b1[:n], mid, vec))
        if n:
            a.bonds[h].pos, a.bonds[h].b0, a.bonds[h].b1 = up(pos).data_ptr(), up(b0).data_ptr(), up(b1).data_ptr()
        a.bonds[h].n, a.bonds[h].mid, a.bonds[h].vec = n, mid.data_ptr(), vec.data_ptr()
    c.copies = []
    for h in range(2):
        n = n_copy[h]
        src = rng.integers(-1000, 1000, max(n, 1)).astype(np.int32)
        dst = torch.full((n + 5,), int(ISENT), dtype=torch.int32, device=dev)
        c.copies.append((src[:n], dst))
        if n:
            a.copy[h].src = up(src).data_ptr()
        a.copy[h].dst, a.copy[h].n = dst.data_ptr(), n
    c.args = a
    return c


def _prologue_check(c, dev, what):
    """With u = 2^-24, eps_pow = 2 x the powf yardstick (relative), eps_sin = 2 x the sin / cos yardstick (absolute):
      sigma   = min^(1 - t) max^t (1 - t is exact for t = i / 4096): two powf and a product    <= (2 eps_pow + 2 u) sigma
      cut     = sigma mul + add, rounded twice                                                <= dsigma |mul| + 2 u (|sigma mul| + |add|);
                from an INPUT sigma it is the float32 expression bit for bit
      emb     sin / cos of the float32 argument (1000 t) freq[s] (both products float32, as the definition forms it)  <= eps_sin;
                the zero column of an odd sd exact
      centre  an n-term float32 sum in some order, one division                               <= (n + 2) u sum |x_p| / n; an empty graph: +0.0
      mid, vec, the copies: bit for bit the float32 expressions; everything behind n_graphs / n keeps its sentinel."""
    B = c.B
    eps_pow, eps_sin = 2.0 * _pow_yardstick(dev), 2.0 * _sincos_yardstick(dev)
    t64 = c.t.astype(F64)
    sig64, dsig = [None] * 4, [None] * 4
    for k in range(4):
        got = c.d_sig[k].cpu().numpy()
        if c.modes[k] == "n":
            assert _is_sentinel(got), f"{what}: sigma[{k}] is NULL, its neighbour buffer was written"
            continue
        assert _is_sentinel(got[B:]), f"{what}: sigma[{k}] behind n_graphs"
        if c.modes[k] == "i":
            assert np.array_equal(_bits(got[:B]), _bits(c.sig_in[k, :B])), f"{what}: an input sigma[{k}] changed"
            sig64[k], dsig[k] = c.sig_in[k, :B].astype(F64), np.zeros(B)
        else:
            lo, hi = float(np.float32(_SIG_RANGES[k][0])), float(np.float32(_SIG_RANGES[k][1]))
            sig64[k] = lo ** (1.0 - t64[:, k]) * hi ** t64[:, k]
            dsig[k] = (2 * eps_pow + 2 * U24) * sig64[k]
            _assert_within(got[:B], sig64[k], dsig[k], f"{what} sigma[{k}]")
    cut = c.d_cut.cpu().numpy()
    if c.modes[0] == "n":
        assert _is_sentinel(cut)
    else:
        assert _is_sentinel(cut[B:])
        mul, add = float(c.cut_mul), float(c.cut_add)
        _assert_within(cut[:B], sig64[0] * mul + add, dsig[0] * mul + 2 * U24 * (np.abs(sig64[0] * mul) + add), f"{what} cut")
        s32 = c.d_sig[0].cpu().numpy()[:B]                    # (an extra: the cutoff follows the sigma that was written)
        assert np.array_equal(_bits(cut[:B]), _bits((s32 * c.cut_mul).astype(np.float32) + c.cut_add)), f"{what}: cut is not sigma * mul + add in float32"
    emb = c.d_emb.cpu().numpy()
    if not c.with_emb:
        assert _is_sentinel(emb)
    else:
        assert _is_sentinel(emb[B:])
        if B:
            half = c.sd // 2
            arg = _emb_args(c.t[:, 0], c.freq).astype(F64)
            want = np.concatenate([np.sin(arg), np.cos(arg), np.zeros((B, c.sd - 2 * half))], 1)
            _assert_within(emb[:B], want, np.full(want.shape, eps_sin), f"{what} graph_emb")
            if c.sd & 1:
                assert (_bits(emb[:B, c.sd - 1]) == 0).all(), f"{what}: the zero column of an odd sd"
    cen = c.d_cen.cpu().numpy()
    assert _is_sentinel(cen[B:])
    for g in range(B):
        p = c.lig[c.ptr[g]:c.ptr[g + 1]].astype(F64)
        n = p.shape[0]
        if n == 0:
            assert (_bits(cen[g]) == 0).all(), f"{what}: the centre of an empty graph is not +0.0"
        else:
            _assert_within(cen[g], p.mean(0), (n + 2) * U24 * np.abs(p).sum(0) / n, f"{what} centre of graph {g} ({n} atoms)")
    for h, (pos, b0, b1, mid, vec) in enumerate(c.bonds):
        n = c.n_bonds[h]
        gm, gv = mid.cpu().numpy(), vec.cpu().numpy()
        assert _is_sentinel(gm[n:]) and _is_sentinel(gv[n:]), f"{what}: bonds[{h}] behind n"
        if n:
            with np.errstate(over="ignore"):
                wm, wv = ((pos[b0] + pos[b1]) / np.float32(2)).astype(np.float32), (pos[b1] - pos[b0]).astype(np.float32)
            assert np.isinf(wm[0]).all()
            assert np.array_equal(_bits(gm[:n]), _bits(wm)), f"{what}: bonds[{h}].mid is not (u + v) / 2 in float32"
            assert np.array_equal(_bits(gv[:n]), _bits(wv)), f"{what}: bonds[{h}].vec is not v - u in float32"
    for h, (src, dst) in enumerate(c.copies):
        n = c.n_copy[h]
        g = dst.cpu().numpy()
        assert np.array_equal(g[:n], src) and (g[n:] == ISENT).all(), f"{what}: copy[{h}]"


def _prologue_run(c):
    L, lib, K = _api()
    return lib.ddp_step_prologue(C.byref(c.args), K.stream())


_SECTION_CASES = [((1, 63, 64, 65, 200), (0, 1), (63, 64), 32, 1, "cccc"),
                  ((65,), (65, 130), (0, 1), 33, 0, "cinc"),
                  ((), (63, 64), (65, 130), 2, 1, "cccc"),
                  ((1, 63, 64, 65, 200), (64, 0), (130, 65), 64, 4, "icni"),
                  ((65,), (130, 65), (64, 0), 2, 4, "ccci"),
                  ((), (1, 63), (1, 63), 33, 0, "nccn"),
                  ((1, 63, 64, 65, 200), (0, 0), (0, 0), 33, 0, "ncic"),
                  ((), (0, 0), (0, 0), 32, 1, "cccc")]


@pytest.mark.parametrize("i", range(len(_SECTION_CASES)))
def test_prologue_all_sections_in_one_launch(i):
    """The graph section and the four sections behind it - bonds[0], bonds[1], copy[0], copy[1] - present together, their lengths
    drawn from {0, 1, 63, 64, 65, 130} (every section once empty and once exactly one block), n_graphs in {0, 1, 5} with graphs of
    1, 63, 64, 65 and 200 atoms (the centre's 64-lane stride wraps), sd in {2, 32, 33, 64}, t_stride 0 / 1 / 4 (interleaved times),
    sigma[k] computed / an input / NULL mixed in one call."""
    dev = _dev()
    sizes, nb, nc, sd, ts, modes = _SECTION_CASES[i]
    c = _prologue_case(i, dev, sizes, nb, nc, sd, ts, modes)
    assert _prologue_run(c) == 0
    _prologue_check(c, dev, f"prologue[{i}]")


def test_prologue_empty_graph_has_a_zero_centre():
    """graph_ptr[g] == graph_ptr[g + 1]: the mean over no atoms is the zero vector (torch_scatter's mean, which the kernel replaces,
    divides by the count clamped to 1) - not 0 / 0.  First, middle and last graph empty."""
    dev = _dev()
    c = _prologue_case(77, dev, (0, 3, 0, 70, 0), (5, 0), (0, 9), 32, 1, "cccc")
    assert _prologue_run(c) == 0
    _prologue_check(c, dev, "prologue, empty graphs")


def test_prologue_refuses_what_it_cannot_run():
    """cut without sigma[0]; graph_emb with sd < 2; a bond job with n > 0 and a null pointer: an error code, nothing written."""
    dev = _dev()
    for what in ("cut", "sd", "bond"):
        c = _prologue_case(5, dev, (4, 9), (3, 3), (2, 2), 32, 1, "nccc" if what == "cut" else "cccc")
        if what == "cut":
            c.args.cut = c.d_cut.data_ptr()
        elif what == "sd":
            c.args.sd = 1
        else:
            c.args.bonds[1].b1 = 0
        assert _prologue_run(c) != 0, what
        torch.cuda.synchronize()
        for t in [c.d_cut, c.d_emb, c.d_cen, c.bonds[0][3], c.bonds[1][4]] + [c.d_sig[k] for k in range(4) if c.modes[k] != "i"]:
            assert _is_sentinel(t), what
        assert all(bool((dst == int(ISENT)).all()) for _, dst in c.copies)


# ====================================================================================================== 3. read-out MLPs
_TRROT_SHAPES = ((1, 0), (16, 1), (24, 33), (60, 32), (64, 64))
SO3_N, SO3_LO, SO3_HI = 1000, math.log10(0.01), math.log10(2.0)
TORUS_N, TORUS_LO, TORUS_HI = 5000, math.log(3e-3), math.log(2.0)


def _trrot_case(seed, dev, B, ns, sd, ld_gp, sig0, sig1):
    L, lib, K = _api()
    rng = np.random.default_rng(seed)
    c = _Case()
    c.B, c.ns, c.sd = B, ns, sd
    c.gp = rng.standard_normal((B, 12)).astype(np.float32)
    c.emb = rng.standard_normal((B, max(sd, 1))).astype(np.float32)[:, :sd]
    c.w1 = (rng.standard_normal((2, ns, 1 + sd)) * 0.4).astype(np.float32)
    c.b1 = rng.standard_normal((2, ns)).astype(np.float32)
    c.w2 = rng.standard_normal((2, ns)).astype(np.float32)
    c.b2 = rng.standard_normal((2, 1)).astype(np.float32)
    c.sigma = [(rng.random(B) + 0.2).astype(np.float32) if s else None for s in (sig0, sig1)]
    c.t = dict(gp=_up(_padded(c.gp, ld_gp - 12), dev), emb=_up(c.emb if sd else np.full((B, 1), np.nan, np.float32), dev),
               w1=_up(c.w1, dev), b1=_up(c.b1, dev), w2=_up(c.w2, dev), b2=_up(c.b2, dev),
               sig=[_up(s, dev) if s is not None else None for s in c.sigma], tab=torch.ones(SO3_N, device=dev),
               out=[_sent((B + 1, 3), dev), _sent((B + 1, 3), dev)])
    r = L.TrRotArgs()
    r.gp, r.ld_gp, r.n_graphs, r.ns, r.sd, r.graph_emb = c.t["gp"].data_ptr(), ld_gp, B, ns, sd, c.t["emb"].data_ptr()
    for h in range(2):
        r.w1[h], r.b1[h], r.w2[h], r.b2[h] = (c.t[k][h].data_ptr() for k in ("w1", "b1", "w2", "b2"))
        r.sigma[h] = K._p(c.t["sig"][h])
        r.out[h] = c.t["out"][h].data_ptr()
    r.so3_table, r.so3_n, r.so3_lo, r.so3_span = c.t["tab"].data_ptr(), SO3_N, float(np.float32(SO3_LO)), float(np.float32(SO3_HI - SO3_LO))
    c.args = r
    return c


def _trrot_check(c, what):
    """out = v / |v| * MLP([|v|, emb]) (/ sigma_tr; the so3 table is all ones) in float64.  With u = 2^-24:
      v      = 1o + 1e halves, one add per component: relative u;  |v|: three squares, two adds, a root:   d|v| <= 4 u |v|
      pre_j  = w1[j, 0] |v| + sum_k w1[j, 1 + k] emb[k] + b1[j], a (1 + sd)-term sum and the bias:
                                                         dpre <= (sd + 3) u (sum |w1| |x| + |b1|) + |w1[j, 0]| d|v|
      mlp    = sum_j relu(pre_j) w2[j] + b2 (relu 1-Lipschitz; the products, a tree over the 64 lanes - lanes >= ns add exact
               zeros -, the bias):                        dmlp <= (ns + 2) u (sum (relu + dpre) |w2| + |b2|) + sum dpre |w2|
      out    = (v_c / |v|) mlp (/ sigma): v_c, |v|, two divisions, a product:
                                                         dout <= |v_c| / |v| dmlp / sigma + 9 u |out|
    The first term is ABSOLUTE in sum |w| |x|: the ReLU sum can cancel."""
    B, ns, sd = c.B, c.ns, c.sd
    g = c.gp.astype(F64)
    for h, v in enumerate((g[:, 0:3] + g[:, 6:9], g[:, 3:6] + g[:, 9:12])):
        nrm = np.linalg.norm(v, axis=1)
        x = np.concatenate([nrm[:, None], c.emb.astype(F64)], 1)
        w1, b1, w2, b2 = c.w1[h].astype(F64), c.b1[h].astype(F64), c.w2[h].astype(F64), float(c.b2[h, 0])
        pre = x @ w1.T + b1
        dpre = (sd + 3) * U24 * (np.abs(x) @ np.abs(w1).T + np.abs(b1)) + np.abs(w1[:, 0])[None, :] * (4 * U24 * nrm)[:, None]
        hid = np.maximum(pre, 0.0)
        mlp = hid @ w2 + b2
        dmlp = (ns + 2) * U24 * ((hid + dpre) @ np.abs(w2) + abs(b2)) + dpre @ np.abs(w2)
        f = 1.0 / c.sigma[0].astype(F64) if (h == 0 and c.sigma[0] is not None) else np.ones(B)
        unit = v / nrm[:, None]
        want = unit * (mlp * f)[:, None]
        tol = np.abs(unit) * (dmlp * f)[:, None] + 9 * U24 * np.abs(want)
        got = c.t["out"][h].cpu().numpy()
        assert _is_sentinel(got[B:]), f"{what}: out[{h}] behind n_graphs"
        _assert_within(got[:B], want, tol, f"{what} head {h}")


@pytest.mark.parametrize("ns,sd", _TRROT_SHAPES)
def test_trrot_head_matches_its_fp64_definition(ns, sd):
    """(ns, sd) from (1, 0) to (64, 64) - the last fills the kernel's static LDS array exactly; sd odd and 0 -, ld_gp 12 and 20
    (NaN padding), n_graphs 1 and 130, the four combinations of sigma[0] / sigma[1] given or NULL."""
    L, lib, K = _api()
    dev = _dev()
    combo = 0
    for B in (1, 130):
        for ld_gp in (12, 20):
            for sig0 in (False, True):
                for sig1 in (False, True):
                    c = _trrot_case(1000 * ns + combo, dev, B, ns, sd, ld_gp, sig0, sig1)
                    assert lib.ddp_trrot_head(C.byref(c.args), K.stream()) == 0
                    _trrot_check(c, f"trrot ns={ns} sd={sd} B={B} ld_gp={ld_gp} sigma={int(sig0)}{int(sig1)}")
                    combo += 1


def test_trrot_head_refuses_what_it_cannot_run():
    """ns = 65, sd = 65, ld_gp = 11: an error code, nothing written."""
    L, lib, K = _api()
    dev = _dev()
    for field, value in (("ns", 65), ("sd", 65), ("ld_gp", 11)):
        c = _trrot_case(1, dev, 3, 16, 32, 12, True, True)
        setattr(c.args, field, value)
        assert lib.ddp_trrot_head(C.byref(c.args), K.stream()) != 0, field
        torch.cuda.synchronize()
        assert _is_sentinel(c.t["out"][0]) and _is_sentinel(c.t["out"][1])


_TOR_NS = (1, 16, 60, 64)
_TOR_COMBOS = [(T, wide, sig) for T in (1, 130) for wide in (False, True) for sig in (False, True)]


def _tor_arrays(ns, combo):
    T, wide, sig = _TOR_COMBOS[combo]
    rng = np.random.default_rng(300 + 100 * ns + combo)
    h = rng.standard_normal((T, 2 * ns)).astype(np.float32)
    w1 = (rng.standard_normal((ns, 2 * ns)) * (1.2 / math.sqrt(2 * ns))).astype(np.float32)
    w2 = rng.standard_normal(ns).astype(np.float32)
    return T, wide, sig, rng, h, w1, w2


def _tanh_yardstick(dev):
    """Absolute error of torch.tanh (ROCm, float32) over the float32-rounded pre-activations h w1^T of EVERY torsion-head case
    (the kernel's own pre-activations are these or their neighbours within dacc; tanh is 1-Lipschitz)."""
    args = []
    for ns in _TOR_NS:
        for combo in range(len(_TOR_COMBOS)):
            T, wide, sig, rng, h, w1, w2 = _tor_arrays(ns, combo)
            args.append((h.astype(F64) @ w1.astype(F64).T).astype(np.float32).ravel())
    return _yardstick("tanhf", dev, torch.tanh, np.tanh, [np.concatenate(args)], False)


def _tor_setup(dev, ns, T, ld_h, sig, rng, h, w1, w2):
    L, lib, K = _api()
    G = 7
    t = dict(h=_up(_padded(h, ld_h - 2 * ns), dev), w1=_up(w1, dev), w2=_up(w2, dev), out=_sent((T + 2,), dev),
             sig=_up((rng.random(G) * 3 + 0.02).astype(np.float32), dev), gob=_up(rng.integers(0, G, T).astype(np.int32), dev),
             tab=torch.ones(TORUS_N + 1, device=dev))
    q = L.TorArgs()
    q.h, q.ld_h, q.n_bonds, q.ns, q.w1, q.w2, q.out = t["h"].data_ptr(), ld_h, T, ns, t["w1"].data_ptr(), t["w2"].data_ptr(), t["out"].data_ptr()
    if sig:
        q.sigma, q.graph_of_bond = t["sig"].data_ptr(), t["gob"].data_ptr()
        q.torus_table, q.torus_n, q.torus_lo, q.torus_span = t["tab"].data_ptr(), TORUS_N, float(np.float32(TORUS_LO)), float(np.float32(TORUS_HI - TORUS_LO))
    return t, q


@pytest.mark.parametrize("ns", _TOR_NS)
def test_tor_head_matches_its_fp64_definition(ns):
    """out[b] = w2 . tanh(w1 h[b]) (x sqrt(table) = 1: the torus table is all ones) for ns in {1, 16, 60, 64} and every combination
    of n_bonds 1 / 130, ld_h = 2 ns / 2 ns + 5 (NaN padding), sigma NULL / given (bond b reads graph_of_bond[b]).  With u = 2^-24
    and eps_tanh = 2 x the tanhf yardstick (absolute):
      acc_j = sum_k w1[j, k] h[k], a 2 ns-term sum from 0:              dacc <= (2 ns + 2) u sum |w1| |h|
      tanh is 1-Lipschitz:                                              dth  <= dacc + eps_tanh
      out   = sum_j tanh_j w2[j] (products, a tree over the lanes):     dout <= (ns + 2) u sum (|tanh| + dth) |w2| + sum dth |w2|"""
    L, lib, K = _api()
    dev = _dev()
    eps_tanh = 2.0 * _tanh_yardstick(dev)
    for combo in range(len(_TOR_COMBOS)):
        T, wide, sig, rng, h, w1, w2 = _tor_arrays(ns, combo)
        ld_h = 2 * ns + (5 if wide else 0)
        t, q = _tor_setup(dev, ns, T, ld_h, sig, rng, h, w1, w2)
        assert lib.ddp_tor_head(C.byref(q), K.stream()) == 0
        h64, w164, w264 = h.astype(F64), w1.astype(F64), w2.astype(F64)
        acc = h64 @ w164.T
        dth = (2 * ns + 2) * U24 * (np.abs(h64) @ np.abs(w164).T) + eps_tanh
        th = np.tanh(acc)
        want = th @ w264
        tol = (ns + 2) * U24 * ((np.abs(th) + dth) @ np.abs(w264)) + dth @ np.abs(w264)
        got = t["out"].cpu().numpy()
        assert _is_sentinel(got[T:])
        _assert_within(got[:T], want, tol, f"tor head ns={ns} T={T} ld_h={ld_h} sigma={int(sig)}")


def test_tor_head_refuses_what_it_cannot_run():
    """ld_h < 2 ns; sigma without graph_of_bond: an error code, nothing written."""
    L, lib, K = _api()
    dev = _dev()
    for ns in (1, 60):
        T, wide, sig, rng, h, w1, w2 = _tor_arrays(ns, 1)
        t, q = _tor_setup(dev, ns, T, 2 * ns, True, rng, h, w1, w2)
        q.ld_h = 2 * ns - 1
        assert lib.ddp_tor_head(C.byref(q), K.stream()) != 0
        q.ld_h, q.graph_of_bond = 2 * ns, 0
        assert lib.ddp_tor_head(C.byref(q), K.stream()) != 0
        torch.cuda.synchronize()
        assert _is_sentinel(t["out"])


# ====================================================================================================== 4. side chains, SDE update
_SC_SIZES = (130, 130, 65, 64, 63, 1, 0, 130)    # atoms per subcomponent range: around the kernel's 64-thread stride
_SC_ATOMS = 500


def _sidechain_problem(seed):
    """A synthetic residue set.  Atoms 0 .. 15 are the bonds' axis atoms.  Bond 0 stands alone: it turns a 130-atom range about
    pos[12] - pos[13], two atoms no bond moves, so its bound carries no history and is the tight one.  Bonds 1 .. 7 are a chain:
    chain bond c = j - 1 turns about pos[2c] - pos[2c + 1] through pos[2c + 1] (the last one about pos[9] - pos[8], chain bond
    4's axis reversed), and its range holds the axis atoms of the next chain bond, so every later axis was moved by an earlier
    bond.  Ranges overlap otherwise (atoms 16 .. 399, drawn without repeats inside a range); atoms 400 .. 499 - and 0, 1, 11 .. 15
    - are in no range."""
    rng = np.random.default_rng(seed)
    nc = len(_SC_SIZES) - 1
    chain = [[2 * c, 2 * c + 1] for c in range(nc - 1)] + [[9, 8]]
    edge = np.array([[12, 13]] + chain, np.int32)
    sub, mapping = [], []
    for j, size in enumerate(_SC_SIZES):
        c = j - 1
        nxt = [int(a) for a in chain[c + 1]] if 0 <= c < nc - 2 else []
        must = [a for a in nxt if a not in (int(edge[j][0]), int(edge[j][1]))][:size]
        rest = rng.permutation(np.arange(16, 400))[:size - len(must)]
        atoms = rng.permutation(np.concatenate([np.array(must, np.int64), rest]))
        mapping.append([len(sub), len(sub) + size])
        sub.extend(int(a) for a in atoms)
        assert len(atoms) == size == len(set(atoms.tolist()))
    return edge, np.array(sub, np.int32), np.array(mapping, np.int32)


def _rodrigues64(axis, theta):
    n = axis / np.linalg.norm(axis, axis=1, keepdims=True)
    K = np.zeros(axis.shape[:1] + (3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -n[:, 2], n[:, 1], n[:, 2], -n[:, 0], -n[:, 1], n[:, 0]
    s, cc = np.sin(theta)[:, None, None], (1 - np.cos(theta))[:, None, None]
    return np.eye(3)[None] + s * K + cc * (K @ K)


def _sidechain_ref(pos32, ang32, edge, sub, mapping, n_bonds, eps_trig):
    """modify_sidechains in float64, bonds in list order, with a running bound e[s, a] on the Euclidean error of every atom and
    ed[j] on the error of every later bond's axis VECTOR p[u_j] - p[v_j].  u = 2^-24; eps_trig = eps_sin + eps_cos, each 2 x the
    torch-against-float64 yardstick on the test's own angles.  For bond i with axis A of length l, angle th, and an atom x of its
    range at r = |x - p[v]|, the kernel forms w = A (th / l) and the Rodrigues matrix I + a K(w) + b K(w)^2 of w:
      direction of w: A carries ed[i] and one rounding per component, the product with th / l another:  dn <= ed[i] / l + 4 u;
        rotations by one angle about axes dn apart differ by <= 2 dn in norm (R' = Q R Q^T, |Q - I| <= dn);
      angle |w|: l (three squares, two adds, a root, on rounded components: 4 u), the division, the products: relative 10 u, and a
        rotation about one axis by angles 10 u |th| apart differs by that much;
      the matrix of the float32 w as given, entry by entry, ang = |w| again relative 3 u:
        a w_c = sin(ang) n_c:            eps_sin + 3 u |th| (argument) + 5 u (a = sin / ang, the product; |sin| <= 1)
        b w_i w_j = (1 - cos(ang)) n_i n_j, |n_i n_j| <= 1/2 off the diagonal:
                                         (eps_cos + 3 u |th| + 2 u + 10 u (1 - cos)) / 2 <= (eps_cos + 3 u |th| + 22 u) / 2
        off-diagonal entry, with its sum: eps_sin + eps_cos / 2 + 4.5 u |th| + 17 u
        diagonal entry 1 - b (w_j^2 + w_k^2): eps_cos + 3 u |th| + 25 u
        each <= eps_trig + 4.5 u |th| + 25 u, nine of them: Frobenius (>= spectral) norm <= 3 (eps_trig + 4.5 u |th| + 25 u);
      together dR = 2 dn + 3 (eps_trig + 25 u) + 23.5 u |th|;
      x' = R (x - p[v]) + p[v]: the rotation keeps the norm of the incoming error e[x] + e[v]; p[v] adds e[v]; the subtraction,
      the three 3-term dot products and the final add round, rnd(x) = 8 u r + u |x'|:
      e[x'] <= e[x] + 2 e[v] + dR r + rnd(x);
      a later axis whose TWO atoms are both in the range turns as a rigid vector - what the two atoms share cancels in the
      difference: ed[j] <= ed[j] + dR |axis_j| + rnd(u_j) + rnd(v_j); with one atom in the range: ed[j] = e[u_j] + e[v_j] from then on."""
    p = pos32.astype(F64).copy()
    S = p.shape[0]
    e = np.zeros(p.shape[:2])
    ed = [np.zeros(S) for _ in range(n_bonds)]
    rigid = [True] * n_bonds
    for i in range(n_bonds):
        u, v = int(edge[i][0]), int(edge[i][1])
        axis = p[:, u] - p[:, v]
        ln = np.linalg.norm(axis, axis=1)
        th = ang32[:, i].astype(F64)
        R = _rodrigues64(axis, th)
        dax = ed[i] if rigid[i] else e[:, u] + e[:, v]
        dR = 2 * (dax / ln + 4 * U24) + 3 * (eps_trig + 25 * U24) + 23.5 * U24 * np.abs(th)
        idx = sub[mapping[i][0]:mapping[i][1]]
        if idx.size == 0:
            continue
        x = p[:, idx] - p[:, v][:, None, :]
        r = np.linalg.norm(x, axis=2)
        new = np.einsum("sij,saj->sai", R, x) + p[:, v][:, None, :]
        rnd = 8 * U24 * r + U24 * np.linalg.norm(new, axis=2)
        e[:, idx] = e[:, idx] + 2 * e[:, v][:, None] + dR[:, None] * r + rnd
        where = {int(a): k for k, a in enumerate(idx)}
        for j in range(i + 1, n_bonds):
            uj, vj = int(edge[j][0]), int(edge[j][1])
            if uj in where and vj in where:
                ed[j] = ed[j] + dR * np.linalg.norm(p[:, uj] - p[:, vj], axis=1) + rnd[:, where[uj]] + rnd[:, where[vj]]
            elif uj in where or vj in where:
                rigid[j] = False
        p[:, idx] = new
    assert S == ang32.shape[0]
    return p, e


@pytest.mark.parametrize("n_samples", [1, 40])
def test_sidechain_update_matches_its_fp64_definition(n_samples):
    """Ranges of 0, 1, 63, 64, 65 and 130 atoms, one bond that stands alone and a chain of bonds whose axes were moved by earlier
    bonds, against the float64 definition with the running bound of _sidechain_ref (the kernel's sinf / cosf: twice the yardstick
    of torch.sin / torch.cos on the test's |angles|); the in-place and the out-of-place call give the same bits; atoms in no
    range keep their bits; n_bonds = 0 is an exact copy."""
    L, lib, K = _api()
    dev = _dev()
    rng = np.random.default_rng(n_samples)
    edge, sub, mapping = _sidechain_problem(9)
    nb = len(_SC_SIZES)
    pos = (rng.standard_normal((n_samples, _SC_ATOMS, 3)) * 1.5 + rng.standard_normal((n_samples, 1, 3)) * 10).astype(np.float32)
    for j in range(8):                                  # bond lengths of 1.5
        d = rng.standard_normal((n_samples, 3))
        pos[:, 2 * j + 1] = pos[:, 2 * j] + (1.5 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    ang = (rng.standard_normal((n_samples, nb)) * 0.8).astype(np.float32)
    eps_trig = 2.0 * (_yardstick(f"sinf (side chains, {n_samples})", dev, torch.sin, np.sin, [np.abs(ang).ravel()], False)
                      + _yardstick(f"cosf (side chains, {n_samples})", dev, torch.cos, np.cos, [np.abs(ang).ravel()], False))
    want, e = _sidechain_ref(pos, ang, edge, sub, mapping, nb, eps_trig)
    want1, e1 = _sidechain_ref(pos, ang[:, :1], edge, sub, mapping, 1, eps_trig)       # the stand-alone bond by itself
    print(f"[fp64] sidechain_update: largest bound of the stand-alone bond {e1.max():.3e}, of the whole problem {e.max():.3e}")
    moved = np.zeros(_SC_ATOMS, bool)
    moved[sub] = True
    assert moved[2:11].all() and not moved[400:].any() and not moved[:2].any() and not moved[11:16].any()
    d_in, d_ang = _up(pos, dev), _up(ang, dev)
    d_edge, d_sub, d_map = _up(edge, dev), _up(sub, dev), _up(mapping, dev)
    out = _sent((n_samples + 1, _SC_ATOMS, 3), dev)

    def run(src, dst, n_bonds):
        return lib.ddp_sidechain_update(src.data_ptr(), n_samples, _SC_ATOMS, d_ang.data_ptr(), n_bonds, d_edge.data_ptr(), d_sub.data_ptr(),
                                        d_map.data_ptr(), dst.data_ptr(), K.stream())

    assert run(d_in, out, nb) == 0
    got = out.cpu().numpy()
    assert _is_sentinel(got[n_samples:]), "a sample behind n_samples was written"
    got = got[:n_samples]
    assert float(np.abs(want - pos).max()) > 1.0                      # (something moved)
    assert np.array_equal(_bits(got[:, ~moved]), _bits(pos[:, ~moved])), "an atom outside every subcomponent range changed"
    _assert_within(got[:, moved], want[:, moved], np.repeat(e[:, moved, None], 3, axis=2), f"sidechain_update, {n_samples} samples")
    first = sub[mapping[0][0]:mapping[0][1]]
    d_ang_all, d_ang = d_ang, _up(ang[:, :1].copy(), dev)                # (angles are [n_samples][n_bonds]: one column for n_bonds = 1)
    out.fill_(float(SENTINEL))
    assert run(d_in, out, 1) == 0
    got1 = out.cpu().numpy()[:n_samples]
    _assert_within(got1[:, first], want1[:, first], np.repeat(e1[:, first, None], 3, axis=2), f"sidechain_update, the stand-alone bond, {n_samples} samples")
    rest = np.ones(_SC_ATOMS, bool)
    rest[first] = False
    assert np.array_equal(_bits(got1[:, rest]), _bits(pos[:, rest]))
    d_ang = d_ang_all
    inplace = d_in.clone()
    assert run(inplace, inplace, nb) == 0
    assert np.array_equal(_bits(inplace), _bits(got)), "in place and out of place differ"
    out.fill_(float(SENTINEL))
    assert run(d_in, out, 0) == 0
    assert np.array_equal(_bits(out[:n_samples]), _bits(pos)) and _is_sentinel(out[n_samples:]), "n_bonds = 0 is not an exact copy"


_SDE_NS = [tuple(int(v) for v in np.roll(base, r)) for base in ((257, 255, 1, 0), (256, 0, 255, 1)) for r in range(4)]


@pytest.mark.parametrize("z_null", [0, 1])
@pytest.mark.parametrize("ns", _SDE_NS)
def test_sde_update_is_the_float32_expression(ns, z_null):
    """out[k][i] = a_k score[k][i] + b_k z[k][i] with both products and the sum rounded separately - numpy float32, bit for bit -
    and a_k score alone where z[k] is NULL (the ODE branch); n[k] in {0, 1, 255, 256, 257} with the largest component at each of
    the four positions (the grid is sized by it), n[k] = 0 with null pointers; memory behind n[k] keeps the sentinel.  z is NULL
    for the components k with k % 2 == z_null: every size tuple runs with both patterns, so each component - the 256- and
    257-long ones that reach the second 256-thread block included - is checked with and without noise."""
    L, lib, K = _api()
    dev = _dev()
    rng = np.random.default_rng(sum(n * 7 ** k for k, n in enumerate(ns)) + z_null)
    coef = rng.standard_normal(8).astype(np.float32)
    d_coef = _up(coef, dev)
    a = L.SdeArgs()
    keep, want = [], []
    for k, n in enumerate(ns):
        a.n[k] = n
        if n == 0:
            want.append(None)
            continue
        s, z = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        out = _sent((n + 3,), dev)
        t = (_up(s, dev), _up(z, dev), out)
        keep.append(t)
        a.score[k], a.out[k] = t[0].data_ptr(), out.data_ptr()
        p = (coef[2 * k] * s).astype(np.float32)
        if k % 2 == z_null:
            want.append((out, p))
        else:
            a.z[k] = t[1].data_ptr()
            want.append((out, (p + (coef[2 * k + 1] * z).astype(np.float32)).astype(np.float32)))
    assert lib.ddp_sde_update(d_coef.data_ptr(), C.byref(a), K.stream()) == 0
    for k, w in enumerate(want):
        if w is not None:
            got = w[0].cpu().numpy()
            assert np.array_equal(_bits(got[:ns[k]]), _bits(w[1])), f"component {k} (n = {ns[k]}) is not the float32 expression"
            assert _is_sentinel(got[ns[k]:]), f"component {k}: memory behind n was written"
    # a component with n > 0 and a null score is refused, nothing written
    for t in keep:
        t[2].fill_(float(SENTINEL))
    k = int(np.argmax(ns))
    a.score[k] = 0
    assert lib.ddp_sde_update(d_coef.data_ptr(), C.byref(a), K.stream()) != 0
    torch.cuda.synchronize()
    assert all(_is_sentinel(t[2]) for t in keep)
