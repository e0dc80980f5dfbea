"""launch.conv_path: the one decision of how each conv runs (ddp_conv_rows or ddp_conv_messages, and in which form), and launch_convs'
dispatch on it.  CPU only: the packs are built on the CPU and the library is a recording stand-in."""
import itertools

import pytest
import torch

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import engine as E
from diffdock_pocket_amd import launch as K
from diffdock_pocket_amd import packing as P
from diffdock_pocket_amd.graph import EdgeView
from diffdock_pocket_amd.score_model import TensorProductScoreModel
from oracle.cases import CASES

CPU = torch.device("cpu")


def _model():
    case = CASES["cfg2_small"]
    kw = dict(case.model_kwargs())
    kw.update(case.ctor_extras())
    kw["device"] = CPU
    return TensorProductScoreModel(**kw)


@pytest.fixture
def switches(monkeypatch):
    """CONV_H2 / CONV_ROWS as the test leaves them are put back afterwards."""
    monkeypatch.setattr(K, "CONV_H2", K.CONV_H2)
    monkeypatch.setattr(K, "CONV_ROWS", K.CONV_ROWS)


def _factorised(m):
    return [K.conv_path(c.packed_g(CPU), m.rows_all_or_none(CPU)) for c in m.conv_layers]


def _direct(m, nsplit=1):
    return [[K.conv_path(pk) for pk in E.direct_packs([(c, nsplit)], CPU)[0]] for c in m.conv_layers]


def test_conv_path_table_of_every_conv(switches):
    """Every conv of cfg2_small (ns = 60: all of them shapes of the row-stationary kernel) under each combination of the switches, read
    when the decision is made: packs are built once per option set and CONV_H2 / CONV_ROWS flip between decisions on the same packs."""
    m = _model()
    assert len(m.conv_layers) == 54 and all(P.rows_supported(c.spec_g) and P.rows_supported(c.spec) for c in m.conv_layers)
    for r16, g3, drows in itertools.product((False, True), repeat=3):
        m.rows_mfma16, m.g_planes3, m.direct_rows = r16, g3, drows
        for h2, rows in itertools.product((False, True), repeat=2):
            K.CONV_H2, K.CONV_ROWS = h2, rows
            want_f = K.ConvPath(True, True, int(r16), int(g3)) if (h2 and rows) else K.ConvPath(False, h2)
            # (the direct convs: only in the 16x16x32 form, the fc.3 bias in k)
            want_d = K.ConvPath(True, True, 1, 0, 1) if (h2 and rows and r16 and drows) else K.ConvPath(False, h2)
            assert _factorised(m) == [want_f] * 54, (r16, g3, drows, h2, rows)
            assert _direct(m) == [[want_d]] * 54, (r16, g3, drows, h2, rows)
            assert K.conv_path(m.final_conv.packed(CPU)) == K.ConvPath(False, h2 and P.h2_steps(m.final_conv.spec) > 0)
    # a direct conv as three tasks of segment ranges: each task's range and stream tiles
    K.CONV_H2, K.CONV_ROWS = True, True
    ranges = P.rows_split_segments(m.conv_layers[8].spec, 3)
    assert _direct(m, 3)[8] == [K.ConvPath(True, True, 1, 0, 1, (a, b), m.conv_layers[8].spec.nct1 + n) for a, b, n in ranges]


def test_a_weight_beyond_the_planes_moves_every_factorised_conv_to_messages(switches):
    K.CONV_H2, K.CONV_ROWS = True, True
    m = _model()
    with torch.no_grad():
        m.conv_layers[12].fc[0].weight[0, 0] = 300.0        # |w| > 255: beyond ddp_conv_rows' unified planes
    m.invalidate_packed()
    assert m.conv_layers[12].packed_g(CPU).wsh is None and m.conv_layers[13].packed_g(CPU).wsh is not None
    assert not m.rows_all_or_none(CPU)
    assert _factorised(m) == [K.ConvPath(False, True)] * 54
    # (the direct convs are decided per launch: only the conv that cannot pack leaves the rows kernel)
    assert [d[0].rows for d in _direct(m)] == [i != 12 for i in range(54)]


def test_a_bias_beyond_stage_a_planes_falls_back_instead_of_raising(switches):
    """packed_g checks stage A's planes next to the weight stream: the fc.3 bias rides in G's Gb columns, at 256 x its value."""
    K.CONV_H2, K.CONV_ROWS = True, True
    m = _model()
    conv = m.conv_layers[21]
    with torch.no_grad():
        conv.fc[3].bias.fill_(1.0e4)
    m.invalidate_packed()
    # (the weights alone pass the rows kernel's check; the right-hand sides of stage A in plane form do not)
    P.rows_stream(conv.spec_g, conv.fc[0].weight, conv.fc[0].bias, conv.fc[3].weight, conv.fc[3].bias, form=conv.rows_form)
    wgh, _, _ = P.factor_weights_gh(conv.spec_g, conv.fc[3].weight, conv.fc[3].bias, fmt=conv.gh_fmt, form=conv.rows_form)
    with pytest.raises(NotImplementedError):
        P.split_h2(wgh[0].unsqueeze(0), unified_scale=P.GH_SW)
    pk = conv.packed_g(CPU)
    assert pk.wsh is None and not m.rows_all_or_none(CPU)
    path = K.conv_path(pk, m.rows_all_or_none(CPU))
    assert path == K.ConvPath(False, True)
    st = K.stage_a_stack([(0, pk)], conv.spec_g.hid, path).prepare(h2=True, x3=False)      # (fp32 G rows: no plane form)
    assert st.gh is None and st.ld == st.W.shape[2] and len(st.meta) == sum(w is not None for w in pk.wg)


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def _record(self, name, arr, n):
        self.calls.append((name, [(arr[i].n_edges, arr[i].rows_seg0, arr[i].rows_seg1, bool(arr[i].wsh)) for i in range(n)]))
        return 0

    def ddp_conv_rows(self, shape, arr, n, stream):
        return self._record("ddp_conv_rows", arr, n)

    def ddp_conv_messages(self, shape, arr, n, stream):
        return self._record("ddp_conv_messages", arr, n)


@pytest.fixture
def lib(monkeypatch, switches):
    fake = _RecordingLib()
    monkeypatch.setattr(L, "load", lambda: fake)
    monkeypatch.setattr(K, "stream", lambda: None)
    return fake


def _task(pk, path, n_edges=5, g=None):
    z = torch.zeros(64)
    zi = torch.zeros(n_edges, dtype=torch.int32)
    segs = [(z, zi, 60, 60)] * 3
    return K.make_task(pk, path, z, 64, EdgeView(n_edges, zi, zi, zi, None, zi, None), z, segs, z, g=g)


def test_launch_convs_dispatches_on_the_tasks_common_path(lib):
    K.CONV_H2, K.CONV_ROWS = True, True
    m = _model()
    convs = m.conv_layers[9:12]
    ok = m.rows_all_or_none(CPU)
    spec_g = convs[0].spec_g
    rows = [_task(c.packed_g(CPU), K.conv_path(c.packed_g(CPU), ok), g=[torch.zeros(64), torch.zeros(64)]) for c in convs]
    K.launch_convs(spec_g, rows)
    assert lib.calls == [("ddp_conv_rows", [(5, 0, 0, True)] * 3)]
    K.CONV_ROWS = False        # (between two launches, on the same packs)
    msgs = [_task(c.packed_g(CPU), K.conv_path(c.packed_g(CPU), ok)) for c in convs]
    K.launch_convs(spec_g, msgs)
    assert lib.calls[1] == ("ddp_conv_messages", [(5, 0, 0, False)] * 3)
    with pytest.raises(L.DdpError):
        K.launch_convs(spec_g, [rows[0], msgs[1]])
    assert len(lib.calls) == 2


def test_direct_convs_that_cannot_all_pack_run_unsplit_through_messages(lib):
    """factorize_min_degree = 0 puts several direct convs in one launch: split into segment ranges through the rows kernel only where
    every one of them packs for it, otherwise one ddp_conv_messages task per conv (no conv recomputed once per range)."""
    K.CONV_H2, K.CONV_ROWS = True, True
    m = _model()
    a, b = m.conv_layers[9 + 8], m.conv_layers[9 + 5]      # (two convs of layer 1: one shape)
    spec = a.spec

    def launch(convs):
        tasks = [_task(pk, K.conv_path(pk)) for pks in E.direct_packs([(c, 3) for c in convs], CPU) for pk in pks]
        K.launch_convs(spec, tasks)
        return lib.calls[-1]

    ranges = [(s0, s1) for s0, s1, _ in P.rows_split_segments(spec, 3)]
    assert launch([a, b]) == ("ddp_conv_rows", [(5, s0, s1, True) for s0, s1 in ranges] * 2)
    with torch.no_grad():
        b.fc[0].weight[0, 0] = 300.0        # beyond the rows kernel's planes: b cannot pack
    m.invalidate_packed()
    assert launch([a, b]) == ("ddp_conv_messages", [(5, 0, 0, False)] * 2)
