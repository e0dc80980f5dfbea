"""The conv kernels' per-edge messages, element by element, against the float64 definition of tests/conv_ref64.py: ddp_conv_messages
(64-edge direct and 32-edge factorised kernels, fp32 and h2 forms), ddp_conv_rows (both operand images, both plane forms of G) and
ddp_conv_rows16_direct_kernel (one task and three tasks of segment ranges), through the task structure the engine uses - three segment
tensors with their own strides and index arrays, `pos`-mapped rows, several tasks per launch around the 8-XCD tile remap, device-side counts.

Every assertion is |msg - msg64| <= bound on EVERY element, bound = the composition of the documented per-stage bounds written out in
conv_ref64's docstring, multiplier 1 (dense cases), or the sharp probe's (p 2^-21 + 8 2^-24) sum|terms| (sparse inputs; a lost operand plane
is 2^-11 of a term - tests/test_conv_ref64_cpu.py shows the separation on the same inputs without a kernel).  Rows a launch must not touch
hold SENTINEL and are compared bit for bit; entries of index arrays behind a device-side count are IN RANGE and point at all-NaN rows, so a
wrong read shows as a NaN.  The max err / bound lines this file prints are collected in profiles/conv_messages_fp64.txt (a record, not the
source of any tolerance)."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import conv_ref64 as R
from helpers import SENTINEL, _assert_within, _bits, _up

pytestmark = pytest.mark.gpu

GUARD = 8
NAN = float("nan")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda")


def _api():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import launch as K
    from diffdock_pocket_amd import packing as P
    return L, K, P


@contextmanager
def _switches(h2, rows):
    from diffdock_pocket_amd import launch as K
    was = K.CONV_H2, K.CONV_ROWS
    K.CONV_H2, K.CONV_ROWS = h2, rows
    try:
        yield
    finally:
        K.CONV_H2, K.CONV_ROWS = was


# ------------------------------------------------------------------------------------------------ a conv, its weights, its kernel forms
# name: (factorised, CONV_H2, CONV_ROWS, rows_form, gh_fmt, tasks of segment ranges, edge tile of the kernel)
FORMS = {
    "d64_fp32": (False, False, False, 0, 0, 1, 64), "d64_h2": (False, True, False, 0, 0, 1, 64),
    "drows16": (False, True, True, 1, 0, 1, 128), "drows16x3": (False, True, True, 1, 0, 3, 128),
    "f32_fp32": (True, False, False, 0, 0, 1, 32), "f32_h2": (True, True, False, 0, 0, 1, 32),
    "frows_00": (True, True, True, 0, 0, 1, 128), "frows_01": (True, True, True, 0, 1, 1, 128),
    "frows_10": (True, True, True, 1, 0, 1, 128), "frows_11": (True, True, True, 1, 1, 1, 128),
}
ROWS_FORMS = ("frows_00", "frows_01", "frows_10", "frows_11")


class Conv:
    """One TensorProductConvLayer (batch_norm off) on the device, its unpacked weights on the host, its packs per kernel form."""

    def __init__(self, ns, nv, layer, seed=0, kind="layer", weights=None):
        L, K, P = _api()
        from diffdock_pocket_amd.score_model import TensorProductConvLayer
        torch.manual_seed(1000 * ns + 10 * layer + seed)
        self.ns, self.kind = ns, kind
        mi = P.irreps_muls(ns, nv, layer)
        self.in_mul, self.d_in = mi, P.irreps_dim(mi)
        if kind == "layer":
            mo = P.irreps_muls(ns, nv, layer + 1)
            spec, spec_g = P.faster_tp_spec(mi, mo, 3 * ns), P.faster_tp_spec(mi, mo, 3 * ns, factorized=True)
            blocks = [(m, d, s) for m, d, s in ((mo[0], 1, True), (mo[1], 3, False), (mo[2], 3, False), (mo[3], 1, False)) if m]
        elif kind == "final":      # (score_model.py: final_conv)
            spec, spec_g, blocks = P.faster_tp_spec(mi, (0, 2, 2, 0), 2 * ns), None, [(2, 3, False), (2, 3, False)]
        else:                      # (score_model.py: tor_bond_conv / sc_tor_bond_conv)
            spec, spec_g, blocks = P.torsion_tp_spec(mi, ns, 3 * ns), None, [(ns, 1, False), (ns, 1, True)]
        self.spec, self.spec_g = spec, spec_g
        self.layer = TensorProductConvLayer(spec, blocks, batch_norm=False, spec_g=spec_g)      # (nn.Linear's own initialisation)
        if weights is not None:
            with torch.no_grad():
                for p, w in zip((self.layer.fc[0].weight, self.layer.fc[0].bias, self.layer.fc[3].weight, self.layer.fc[3].bias), weights):
                    p.copy_(torch.from_numpy(w))
        fc = self.layer.fc
        self.W = tuple(t.detach().numpy().copy() for t in (fc[0].weight, fc[0].bias, fc[3].weight, fc[3].bias))
        self.layer = self.layer.to(_dev())
        self._packs = {}

    def forms(self):
        """The kernel forms this shape admits."""
        L, K, P = _api()
        out = ["d64_fp32"]
        if P.h2_steps(self.spec) > 0:
            out.append("d64_h2")
        if self.kind == "layer" and P.rows_supported(self.spec):
            out += ["drows16", "drows16x3"]
        if self.spec_g is not None:
            out.append("f32_fp32")
            if P.h2_steps(self.spec_g) > 0:
                out.append("f32_h2")
            if P.rows_supported(self.spec_g):
                out += list(ROWS_FORMS)
        return out

    def packs(self, name):
        """(packs: one per task of the conv, the ConvPath they run by, the spec of the launch) - and the assertion that conv_path names
        the form asked for."""
        if name in self._packs:
            return self._packs[name]
        L, K, P = _api()
        fact, h2, rows, rform, gfmt, nsplit, _ = FORMS[name]
        dev, lay = _dev(), self.layer
        with _switches(h2, rows):
            if fact:
                lay.rows_form, lay.gh_fmt, lay._packed_g = rform, gfmt, None
                pks = [lay.packed_g(dev)]
                lay._packed_g = None
            elif rows:
                lay.rows_form, lay.direct_rows = 1, True
                got = lay.packed_rows_direct(dev, nsplit=nsplit)
                assert got is not None, name
                pks = list(got) if nsplit > 1 else [got]
                assert len(pks) == nsplit
            else:
                pks = [lay.packed(dev)]
            paths = [K.conv_path(pk) for pk in pks]
        for path in paths:
            assert path.rows == rows and path.h2 == h2, (name, path)
            if rows:
                assert path.rows_form == rform and path.gh_fmt == gfmt and path.rows_bias_k == (0 if fact else 1), (name, path)
        if nsplit > 1:      # (disjoint ranges of output segments that cover them all)
            segs = sorted(p.rows_seg for p in paths)
            assert segs[0][0] == 0 and all(a[1] == b[0] for a, b in zip(segs[:-1], segs[1:])) and segs[-1][1] == len(P.rows_segments(self.spec))
        self._packs[name] = (pks, paths, self.spec_g if fact else self.spec)
        return self._packs[name]

    def ref_form(self, name):
        fact, h2, rows, _, gfmt, _, _ = FORMS[name]
        return R.Form("rows" if rows else "h2" if h2 else "fp32", fact, gfmt if (fact and rows) else 0)


_CONVS = {}


def _conv(ns, nv, layer, seed=0, kind="layer"):
    key = (ns, nv, layer, seed, kind)
    if key not in _CONVS:
        _CONVS[key] = Conv(ns, nv, layer, seed, kind)
    return _CONVS[key]


# ------------------------------------------------------------------------------------------------ an edge set as a kernel task sees it
class Edges:
    """E listed edges of one conv with everything a task points at.  Host side (float32 values as float64 arrays, in listing order): ea
    [E, F], xs = x[src] [E, D_in], sh [E, 4].  Device side, plain: one edge_attr_ array read as column ranges, x with ldx = D_in, identity eid /
    pos.  engine=True: one tensor per segment with row strides ns / ldx / ldx and its own index array, eid a permutation into longer sh / segment
    arrays, ldx_src > D_in, `pos` a permutation (factorised), and NaN in every unused column and in every row no index names.  `tail` more
    entries follow the E live ones in every index array (for device-side counts): in range, pointing at all-NaN rows.  msg holds SENTINEL and
    GUARD more rows than the capacity."""

    def __init__(self, conv, E, N, seed, fact, engine=False, src=None, tail=0, sh4=None):
        dev = _dev()
        rng = np.random.default_rng(seed)
        spec, ns = conv.spec, conv.ns
        F, D = spec.f_in, conv.d_in
        self.E, self.cap, self.N = E, E + tail, N
        f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731
        x = f32(rng.normal(size=(N, D)))
        if src is None:
            src = rng.integers(0, N, E)
            src = np.sort(src) if fact else src
        src = np.asarray(src, dtype=np.int64)
        ea = f32(rng.normal(size=(E, F)))
        if sh4 is None:
            v = rng.normal(size=(E, 3))
            sh4 = np.concatenate([np.ones((E, 1)), np.sqrt(3.0) * v / np.linalg.norm(v, axis=1, keepdims=True)], 1)
        sh4 = f32(sh4)
        self.ea, self.xs, self.sh, self.src, self.x = ea.astype(np.float64), x[src].astype(np.float64), sh4.astype(np.float64), src, x
        nseg, w = F // ns, ns
        ldx = (D + 3) // 4 * 4 + 8 if engine else D
        # node rows: [x | NaN columns], then one all-NaN row (the tail's source); engine: nodes without an edge are NaN as well
        xd = np.full((N + 1, ldx), NAN, dtype=np.float32)
        xd[:N, :D] = x
        if engine:
            xd[np.setdiff1d(np.arange(N), src)] = NAN
        self.ldx = ldx
        if engine:
            M = E + 3
            eid = rng.permutation(M)[:E]
            idx = [eid] + [rng.integers(0, N + 2, E) for _ in range(nseg - 1)]
            lds = [w] + [ldx] * (nseg - 1)
            if conv.kind == "torsion":
                lds[2] = w          # (engine._torsion_head: e_t [*, ns], x [*, ldx], bond_attr [*, ns])
            tens = []
            for k in range(nseg):
                rows = M + 1 if k == 0 else N + 3
                tens.append(np.full((rows, lds[k]), NAN, dtype=np.float32))
            # (several edges may name one row of the receiver / source tensors: the row's values are drawn once, edge_attr_ is read back)
            for k in range(nseg):
                rows_used = np.unique(idx[k])
                tens[k][rows_used, :w] = f32(rng.normal(size=(len(rows_used), w)))
                ea[:, k * w:(k + 1) * w] = tens[k][idx[k], :w]
            self.ea = ea.astype(np.float64)
            shd = np.full((M + 1, 4), NAN, dtype=np.float32)
            shd[eid] = sh4
            nan_row = [M] + [N + 2] * (nseg - 1)
            sh_nan = M
        else:
            ead = np.full((E + 1, F), NAN, dtype=np.float32)
            ead[:E] = ea
            eid = np.arange(E)
            idx, lds = [eid] * nseg, [F] * nseg
            tens = None
            shd = np.full((E + 1, 4), NAN, dtype=np.float32)
            shd[:E] = sh4
            nan_row, sh_nan = [E] * nseg, E
        pad = lambda a, v: np.concatenate([a, np.full(tail, v, dtype=np.int64)]).astype(np.int32)      # noqa: E731
        self.x_dev, self.sh_dev = _up(xd, dev), _up(shd, dev)
        self.src_dev, self.eid_dev = _up(pad(src, N), dev), _up(pad(eid, sh_nan), dev)
        if engine:
            self.seg_t = [_up(t, dev) for t in tens]
            self.segs = [(self.seg_t[k], _up(pad(idx[k], nan_row[k]), dev) if k else self.eid_dev, lds[k], w) for k in range(nseg)]
        else:
            self.ea_dev = _up(ead, dev)
            self.segs = [(self.ea_dev[:, k * w:], self.eid_dev, F, w) for k in range(nseg)]
        self.pos = None
        if fact and engine:
            self.pos = rng.permutation(E)
        self.pos_dev = None if self.pos is None else _up(pad(self.pos, 0), dev)      # (the tail's entries name row 0: never written through)
        # (columns no block of the shape covers are the caller's to zero - include/ddp_hip.h, ddp_conv_task_t::msg: the kernels leave them alone)
        self.init_row = np.full(spec.d_out, SENTINEL, dtype=np.float32)
        for c in range(spec.d_out):
            if not any(b.out_off <= c < b.out_off + b.n * b.C for b in spec.blocks):
                self.init_row[c] = 0.0
        self.cnt = None
        self.reset()

    def reset(self):
        self.msg = _up(np.tile(self.init_row, (self.cap + GUARD, 1)), _dev())

    def count(self, n):
        self.cnt = torch.tensor([n], dtype=torch.int32, device=_dev())
        return self

    def live(self):
        return self.E if self.cnt is None else max(0, min(int(self.cnt.item()), self.E))

    def view(self):
        from diffdock_pocket_amd.graph import EdgeView
        return EdgeView(self.cap, self.eid_dev, self.src_dev, self.eid_dev, pos=self.pos_dev, cnt=self.cnt)


def _tasks(conv, name, ed):
    L, K, P = _api()
    pks, paths, spec = conv.packs(name)
    g = conv.layer.node_tensors(pks[0], ed.x_dev, paths[0]) if FORMS[name][0] else None
    ed._keep = g
    return [K.make_task(pk, path, ed.x_dev, ed.ldx, ed.view(), ed.sh_dev, ed.segs, ed.msg, g=g) for pk, path in zip(pks, paths)], spec


_REFS = {}


def _reference(conv, name, ed, probe=False):
    form = conv.ref_form(name)
    key = (id(ed), form)
    if key not in _REFS:
        if len(_REFS) > 8:
            _REFS.clear()
        ref = R.reference(conv.spec, *conv.W, ed.ea, ed.xs, ed.sh, form)
        _REFS[key] = (ref, ed)
    ref = _REFS[key][0]
    bound = R.probe_bound(ref, form) if probe else ref.bound
    assert (bound > 0)[ref.msg != 0].all()      # (the inputs are ones the definition itself can be held to)
    return ref.msg, bound


def _check(conv, name, ed, what, probe=False):
    """The live rows of ed.msg within the bound of the form, every other row (the rows behind a device-side count, the guard rows) SENTINEL
    bit for bit."""
    torch.cuda.synchronize()
    got = ed.msg.cpu().numpy()
    n = ed.live()
    want, bound = _reference(conv, name, ed, probe)
    rows = np.arange(n) if ed.pos is None else ed.pos[:n]
    assert np.isfinite(got[rows]).all(), f"{what}: NaN / inf in a live message row"
    _assert_within(got[rows], want[:n], bound[:n], what)
    rest = np.setdiff1d(np.arange(got.shape[0]), rows)
    bad = [int(r) for r in rest if not np.array_equal(_bits(got[r]), _bits(ed.init_row))]
    assert not bad, f"{what}: rows {bad[:8]} behind the count / in the guard were written"


def _run(conv, name, ed, what, probe=False):
    L, K, P = _api()
    tasks, spec = _tasks(conv, name, ed)
    K.launch_convs(spec, tasks)
    _check(conv, name, ed, f"{what} {name}", probe)
    ed.reset()


# ------------------------------------------------------------------------------------------------ (a) dense cases
E_ALL = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
DENSE = ([((60, 10, 1), E) for E in E_ALL] + [((32, 6, 3), E) for E in E_ALL] + [((60, 10, 0), E) for E in (33, 128, 257)]
         + [((32, 24, 1), E) for E in (31, 129, 257)] + [((24, 6, 1), E) for E in (1, 65, 129)] + [((16, 4, 2), E) for E in (32, 63, 257)]
         + [((20, 4, 1), E) for E in (33, 64, 129)])


@pytest.mark.parametrize("shape,E", DENSE, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_dense_messages_within_the_composed_bound(shape, E):
    """O(1) Gaussian inputs, nn.Linear's weights, every form the shape admits, E on both sides of the 32 / 64 / 128-edge tiles."""
    conv = _conv(*shape)
    N = min(40, max(2, E // 3 + 2))
    names = conv.forms()
    if shape[0] in (24, 16):
        assert set(names) == {"d64_fp32", "d64_h2", "f32_fp32", "f32_h2"}
    if shape[0] == 20:
        assert set(names) == {"d64_fp32", "f32_fp32"}
    if shape == (60, 10, 1):
        assert set(names) == set(FORMS)
    eds = {f: Edges(conv, E, N, seed=E, fact=f) for f in (False, True)}
    for name in names:
        _run(conv, name, eds[FORMS[name][0]], f"dense {shape} E={E}")


# ------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize("kind", ["torsion", "final"])
@pytest.mark.parametrize("ns,nv,layers,E", [(60, 10, 3, 70), (32, 6, 2, 129), (16, 4, 1, 33)])
def test_head_convs(kind, ns, nv, layers, E):
    """tor_bond_conv (DOT-only blocks of sh = [0, t], segments e_t / x / bond_attr with strides ns / ldx / ns) and final_conv (f_in = 2 ns,
    two segments) as the engine builds their tasks, through ddp_conv_messages in the form conv_path picks and in the fp32 form."""
    conv = _conv(ns, nv, layers, kind=kind)
    sh4 = None
    if kind == "torsion":
        t = np.random.default_rng(E).normal(size=(E, 3))
        sh4 = np.concatenate([np.zeros((E, 1)), t], 1)
    ed = Edges(conv, E, 9, seed=E + 1, fact=False, engine=True, sh4=sh4)
    names = conv.forms()
    assert "d64_fp32" in names and not any(FORMS[n][0] or FORMS[n][2] for n in names)
    for name in names:
        _run(conv, name, ed, f"{kind} head ns={ns}")
    # the layer's own entry hands out whole message rows: columns no block covers (the 0o half of a one-layer model's torsion conv) are
    # zero, as the reference's tensor product leaves them.  (Best effort only: a freed SENTINEL-filled block of the same size makes it
    # likely, not certain, that the allocator hands messages() dirty memory; the SENTINEL-initialised msg of the launches above is what
    # pins the kernels' side of the contract.)
    covered = ed.init_row != 0.0
    junk = torch.full((E, conv.spec.d_out), float(SENTINEL), device=_dev())
    del junk
    ei = torch.stack([torch.arange(E) % 5, torch.from_numpy(ed.src)]).to(_dev())
    conv.layer.direct_rows = False      # (through ddp_conv_messages, as the engine runs the heads)
    msg, csr, _ = conv.layer.messages(_up(ed.x, _dev()), ei, _up(ed.ea.astype(np.float32), _dev()), _up(ed.sh.astype(np.float32), _dev()))
    got = msg.cpu().numpy()
    assert np.isfinite(got).all() and (got[:, ~covered] == 0.0).all()
    assert (kind == "torsion" and layers == 1) == bool((~covered).any())


# ------------------------------------------------------------------------------------------------ (b) the sharp probe
_PROBES = {}


def _probe(band):
    if band not in _PROBES:
        L, K, P = _api()
        ns, nv, layer = 60, 10, 1
        mi = P.irreps_muls(ns, nv, layer)
        spec = P.faster_tp_spec(mi, P.irreps_muls(ns, nv, layer + 1), 3 * ns)
        p = R.probe_inputs(spec, P.irreps_dim(mi), mi[0] + mi[1], R.channel_columns(mi), lo=band[0], hi=band[1], seed=1)
        conv = Conv(ns, nv, layer, kind="layer", weights=(p["W1"], p["b1"], p["W2"], p["b2"]))
        _PROBES[band] = (conv, p)
    return _PROBES[band]


class ProbeEdges(Edges):
    def __init__(self, conv, p):
        E = p["ea"].shape[0]
        super().__init__(conv, E, p["x"].shape[0], seed=0, fact=True, src=p["src"], sh4=p["sh"])
        dev = _dev()
        self.ea, self.xs, self.x = p["ea"].astype(np.float64), p["x"][p["src"]].astype(np.float64), p["x"]
        self.ea_dev[:E] = _up(p["ea"], dev)
        self.x_dev[:self.N, :conv.d_in] = _up(p["x"], dev)


@pytest.mark.parametrize("band", [(-3.0, 3.0), (-9.0, -6.0)], ids=["2^-3..2^3", "2^-9..2^-6"])
@pytest.mark.parametrize("name", list(ROWS_FORMS) + ["f32_h2", "drows16"])
def test_sharp_probe_sees_every_operand_plane(name, band):
    """Sparse inputs (conv_ref64.probe_inputs): every message element is a sum of at most three chains of single multiplications, so the
    bound is a few units of 2^-21 of the terms and a dropped hi.lo product, a continuation byte at the wrong exponent or a lo plane at the wrong
    scale (2^-11 ... 2^-12 of a term) falls outside it.  Second band: lo halves subnormal - the header's absolute floors are added."""
    conv, p = _probe(band)
    ed = ProbeEdges(conv, p)
    _run(conv, name, ed, f"probe band {band}", probe=True)


# ------------------------------------------------------------------------------------------------ (c) run structure of the rows kernels
def _runs(which, N):
    last = N - 1
    if which == "distinct32":           # 32 distinct sources in one wave
        return np.arange(32)
    if which == "run40":                # one source for 40 consecutive edges: across the 16-row tile and the wave boundary
        return np.array([0] * 10 + [1] * 40 + list(range(2, 22)))
    if which == "runs_15_16_17":        # (nodes 0, 1, 2, 4 and the last have no edge)
        return np.array([3] * 15 + [5] * 16 + [6] * 17)
    if which == "last_row_new_run":     # a run that starts on the last valid row of a partial wave, its G row the last of the array
        return np.array([0] * 44 + [last])
    if which == "e129":                 # the 129th edge a run of its own (and a workgroup of its own)
        return np.concatenate([np.sort(np.random.default_rng(3).integers(0, last, 128)), [last]])
    raise KeyError(which)


@pytest.mark.parametrize("which", ["distinct32", "run40", "runs_15_16_17", "last_row_new_run", "e129"])
@pytest.mark.parametrize("shape", [(60, 10, 1), (32, 6, 3)], ids=lambda s: "-".join(map(str, s)))
def test_rows_kernels_g_runs(shape, which):
    """The rows kernels take one G pass per run of edges with one source node inside a 32-row wave: run lengths around the 16-row tile,
    runs across wave boundaries, a run on the last valid row, source nodes without edges, the last row of the G array."""
    conv = _conv(*shape)
    N = 34
    src = _runs(which, N)
    ed = Edges(conv, len(src), N, seed=len(src), fact=True, src=src)
    for name in ROWS_FORMS:
        _run(conv, name, ed, f"runs {which} {shape}")


# ------------------------------------------------------------------------------------------------ (d) engine-shaped tasks
@pytest.mark.parametrize("shape", [(60, 10, 1), (32, 6, 3), (24, 6, 1)], ids=lambda s: "-".join(map(str, s)))
def test_engine_shaped_tasks(shape):
    """Three segment tensors (row strides ns / ldx / ldx, ldx_src > D_in) with three index arrays, eid a permutation, NaN in every unused
    column and unnamed row, `pos` a permutation for the factorised tasks, guard rows behind msg."""
    conv = _conv(*shape)
    E, N = 133, 21
    eds = {f: Edges(conv, E, N, seed=7, fact=f, engine=True) for f in (False, True)}
    assert eds[True].ldx > conv.d_in and eds[True].pos is not None
    for name in conv.forms():
        _run(conv, name, eds[FORMS[name][0]], f"engine tasks {shape}")


# ------------------------------------------------------------------------------------------------ (e) several tasks in one launch
def _task_sizes(T, tiles):
    """Edge counts of 9 tasks whose tile count for the edge tile T is `tiles` (7, 8, 9: around the remap over 8 XCDs): one task empty on the
    host, one with a single edge, partial and full tiles among the others."""
    sizes = {7: [T - 1, 0, 1, T, 5, 0, T // 2 + 1, T, 3], 8: [T - 1, 0, 1, T, 5, T, T // 2 + 1, T, 3],
             9: [T - 1, 0, 1, T + 3, 5, T, T // 2 + 1, T, 3]}[tiles]
    assert sum(-(-n // T) for n in sizes) == tiles and len(sizes) == 9
    return sizes


@pytest.mark.parametrize("tiles", [7, 8, 9])
@pytest.mark.parametrize("name", ["f32_h2", "d64_h2", "frows_11", "frows_00"])
def test_nine_tasks_in_one_launch(name, tiles):
    """Nine tasks of one shape with their own weights, inputs and message buffers; a task that is empty on the host passes null arrays."""
    L, K, P = _api()
    shape = (32, 6, 3)
    fact, T = FORMS[name][0], FORMS[name][6]
    sizes = _task_sizes(T, tiles)
    convs = [_conv(*shape, seed=i) for i in range(9)]
    assert not np.array_equal(convs[0].W[2], convs[1].W[2])
    eds, tasks = [], []
    for i, (conv, n) in enumerate(zip(convs, sizes)):
        if n == 0:
            t = L.ConvTask()      # all pointers null, n_edges = 0: nothing of it may be read
            t._path = conv.packs(name)[1][0]
            eds.append(None)
            tasks.append(t)
            continue
        ed = Edges(conv, n, 12, seed=100 * tiles + i, fact=fact, engine=True)
        ts, spec = _tasks(conv, name, ed)
        eds.append(ed)
        tasks += ts
    K.launch_convs(spec, tasks)
    for i, (conv, ed) in enumerate(zip(convs, eds)):
        if ed is not None:
            _check(conv, name, ed, f"9 tasks, {tiles} tiles of {T}, task {i} ({ed.E} edges) {name}")


def test_direct_rows_tasks_of_several_convs_in_one_launch():
    """ddp_conv_rows16_direct_kernel with 9 tasks: three convs (own weights and edges), each as three tasks of segment ranges writing one msg;
    129, 1 and 128 edges: 2 + 1 + 1 tiles of 128 edges per range, 12 workgroups in the launch."""
    L, K, P = _api()
    convs = [_conv(60, 10, 1, seed=i) for i in range(3)]
    eds, tasks = [], []
    for i, (conv, n) in enumerate(zip(convs, (129, 1, 128))):
        ed = Edges(conv, n, 12, seed=50 + i, fact=False, engine=True)
        ts, spec = _tasks(conv, "drows16x3", ed)
        eds.append(ed)
        tasks += ts
    assert len(tasks) == 9
    K.launch_convs(spec, tasks)
    for i, (conv, ed) in enumerate(zip(convs, eds)):
        _check(conv, "drows16x3", ed, f"3 convs x 3 ranges, conv {i} ({ed.E} edges) drows16x3")


# ------------------------------------------------------------------------------------------------ (f) device-side counts
@pytest.mark.parametrize("name", ["d64_h2", "drows16", "f32_h2", "frows_11", "frows_00"])
def test_device_side_counts(name):
    """*n_edges_dev equal to the capacity, below it inside a tile, below it by whole tiles, 0 and above it (clamped); then a launch of three
    tasks of which one carries a count.  The index entries behind the count are in range and name all-NaN rows of x, the segment tensors, sh
    and G: the live rows stay finite and within the bound, the rows at and behind the count keep SENTINEL."""
    L, K, P = _api()
    conv = _conv(60, 10, 1)
    fact, T = FORMS[name][0], FORMS[name][6]
    E = 2 * T + 5
    # (live rows never reach into the tail: its entries name NaN rows.  Capacity E: the count equal to it and above it; capacity E + 3: the
    # count inside the last tile; capacity E + T + 7: below it by whole tiles, and 0)
    for tail, counts in ((0, (E, E + 1000)), (3, (E,)), (T + 7, (E, E - T - 1, 0))):
        ed = Edges(conv, E, 30, seed=11, fact=fact, engine=True, tail=tail)
        for n in counts:
            _run(conv, name, ed.count(n), f"count {n} of capacity {E + tail}")
    tail = T + 7
    # mixed launch: the middle task has a count, the others none
    eds = [Edges(conv, T + 3, 12, seed=20, fact=fact, engine=True), Edges(conv, E, 30, seed=11, fact=fact, engine=True, tail=tail).count(T + 1),
           Edges(conv, 5, 12, seed=22, fact=fact, engine=True)]
    tasks = []
    for e_ in eds:
        ts, spec = _tasks(conv, name, e_)
        tasks += ts
    K.launch_convs(spec, tasks)
    for i, e_ in enumerate(eds):
        _check(conv, name, e_, f"mixed counts, task {i} {name}")


# ------------------------------------------------------------------------------------------------ (g) empty launches
@pytest.mark.parametrize("name", ["d64_h2", "f32_h2", "frows_11", "drows16"])
def test_empty_launches_write_nothing(name):
    L, K, P = _api()
    lib = L.load()
    conv = _conv(60, 10, 1)
    pks, paths, spec = conv.packs(name)
    fn = lib.ddp_conv_rows if paths[0].rows else lib.ddp_conv_messages
    shape = spec.ctypes_shape()
    arr = (L.ConvTask * 1)()
    assert fn(C.byref(shape), arr, 0, K.stream()) == 0                     # zero tasks
    ed = Edges(conv, 5, 4, seed=1, fact=FORMS[name][0])
    ts, _ = _tasks(conv, name, ed)
    for t in ts:
        t.n_edges = 0
    arr = (L.ConvTask * len(ts))(*ts)
    assert fn(C.byref(shape), arr, len(ts), K.stream()) == 0               # every task empty
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ed.msg), _bits(np.tile(ed.init_row, (ed.cap + GUARD, 1))))
