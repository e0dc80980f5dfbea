"""CPU tests of tests/conv_ref64.py: the fp64 definition of the per-edge conv message against the oracle's own float64 forward, and the
bounds of the GPU tests (tests/test_gpu_conv_messages_fp64.py) against emulated operand roundings - right inside, wrong outside - without
a kernel.  The golden fixtures record strided samples of the conv outputs (`conv_stats`), not the tensors: no golden comparison here."""
import numpy as np
import pytest
import torch

import conv_ref64 as R
from helpers import rel_err
from oracle import thirdparty as tp
from oracle.ref_model import OracleConfig, OracleScoreModel, faster_tensor_product

from diffdock_pocket_amd import packing as P


def _fc(spec, seed):
    g = torch.Generator().manual_seed(seed)
    fc0, fc3 = torch.nn.Linear(spec.f_in, spec.hid), torch.nn.Linear(spec.hid, spec.weight_numel)
    with torch.no_grad():
        for p in (*fc0.parameters(), *fc3.parameters()):
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.0 / np.sqrt(p.shape[-1] if p.dim() > 1 else spec.hid)))
    return {"c.fc.0.weight": fc0.weight.detach(), "c.fc.0.bias": fc0.bias.detach(), "c.fc.3.weight": fc3.weight.detach(),
            "c.fc.3.bias": fc3.bias.detach()}


def _inputs(spec, d_in, E, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, d_in, generator=g, dtype=torch.float64)
    src = torch.randint(0, N, (E,), generator=g)
    ea = torch.randn(E, spec.f_in, generator=g, dtype=torch.float64)
    sh = tp.spherical_harmonics("1x0e+1x1o", torch.randn(E, 3, generator=g, dtype=torch.float64), normalize=True, normalization="component")
    return x, src, ea, sh


def _close(got, want, what):
    err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    assert err <= 1e-12, (what, err)


@pytest.mark.parametrize("ns,nv", [(16, 4), (32, 6), (60, 10)])
@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_definition_equals_the_fp64_oracle_on_the_layer_convs(ns, nv, layer):
    cfg = OracleConfig(ns=ns, nv=nv)
    mi, mo = P.irreps_muls(ns, nv, layer), P.irreps_muls(ns, nv, layer + 1)
    spec = P.faster_tp_spec(mi, mo, 3 * ns)
    sd = _fc(spec, 7 + layer)
    x, src, ea, sh = _inputs(spec, P.irreps_dim(mi), 23, 7, ns + layer)
    om = OracleScoreModel(cfg, sd, dtype=torch.float64)
    want = faster_tensor_product(cfg.irreps(layer), cfg.irreps(layer + 1), x[src], sh, om._mlp("c.fc", ea)).numpy()
    ref = R.reference(spec, sd["c.fc.0.weight"], sd["c.fc.0.bias"], sd["c.fc.3.weight"], sd["c.fc.3.bias"], ea, x[src], sh)
    _close(ref.msg, want, (ns, nv, layer))
    assert bool((ref.bound > 0)[ref.msg != 0].all())


@pytest.mark.parametrize("ns,nv,layers", [(16, 4, 2), (60, 10, 3), (32, 6, 1)])
def test_definition_equals_the_fp64_oracle_on_the_head_convs(ns, nv, layers):
    """final_conv (f_in = 2 ns, "2x1o+2x1e") through faster_tensor_product, the torsion conv through the oracle's
    FullyConnectedTensorProduct over the 20 torsion harmonics - of which the conv reads the 1o block as sh = [0, t]."""
    cfg = OracleConfig(ns=ns, nv=nv, num_conv_layers=layers)
    m_final = P.irreps_muls(ns, nv, layers)
    d_in = P.irreps_dim(m_final)
    fspec = P.faster_tp_spec(m_final, (0, 2, 2, 0), 2 * ns)
    sd = _fc(fspec, 3)
    x, src, ea, sh = _inputs(fspec, d_in, 19, 6, ns)
    om = OracleScoreModel(cfg, sd, dtype=torch.float64)
    want = faster_tensor_product(cfg.irreps(layers), "2x1o+2x1e", x[src], sh, om._mlp("c.fc", ea)).numpy()
    ref = R.reference(fspec, sd["c.fc.0.weight"], sd["c.fc.0.bias"], sd["c.fc.3.weight"], sd["c.fc.3.bias"], ea, x[src], sh)
    _close(ref.msg, want, "final_conv")
    tspec = P.torsion_tp_spec(m_final, ns, 3 * ns)
    sd = _fc(tspec, 4)
    x, src, ea, _ = _inputs(tspec, d_in, 19, 6, ns + 1)
    tor_sh = torch.randn(19, 20, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    om = OracleScoreModel(cfg, sd, dtype=torch.float64)
    fctp = tp.FullyConnectedTensorProduct(cfg.irreps(layers), om.tor_sh_irreps, f"{ns}x0o+{ns}x0e", shared_weights=False)
    w = om._mlp("c.fc", ea)
    assert fctp.weight_numel == w.shape[1] == tspec.weight_numel
    want = fctp(x[src], tor_sh, w).numpy()
    sh4 = torch.cat([torch.zeros(19, 1, dtype=torch.float64), tor_sh[:, :3]], 1)
    ref = R.reference(tspec, sd["c.fc.0.weight"], sd["c.fc.0.bias"], sd["c.fc.3.weight"], sd["c.fc.3.bias"], ea, x[src], sh4)
    _close(ref.msg, want, "torsion conv")


# ------------------------------------------------------------------------------------------------ the bounds, without a kernel
PROBE_FORMS = [R.Form("rows", True, 1), R.Form("rows", True, 0), R.Form("h2", True, 0), R.Form("rows", False, 0)]


def _probe(lo, hi):
    ns, nv, layer = 60, 10, 1
    mi, mo = P.irreps_muls(ns, nv, layer), P.irreps_muls(ns, nv, layer + 1)
    spec = P.faster_tp_spec(mi, mo, 3 * ns)
    return spec, R.probe_inputs(spec, P.irreps_dim(mi), mi[0] + mi[1], R.channel_columns(mi), lo=lo, hi=hi, seed=1)


def _blocks_of(spec, kinds):
    return [b for b in spec.blocks if any(s[0] in kinds for s in b.segs)]


@pytest.mark.parametrize("band", [(-3.0, 3.0), (-9.0, -6.0)])
@pytest.mark.parametrize("form", PROBE_FORMS, ids=lambda f: f"{f.kernel}-{int(f.factorized)}-{f.gh_fmt}")
def test_probe_bound_holds_the_documented_rounding(form, band):
    """The sharp probe's inputs (GPU test (b)) through the emulated operand planes: every element inside the probe bound, in both
    magnitude bands; every chain occurs (all j, k, input channels) and the bound is positive wherever the message is not zero."""
    spec, p = _probe(*band)
    assert len(set(np.nonzero(p["ea"])[1])) == spec.f_in and (np.count_nonzero(p["ea"], axis=1) == 1).all()
    assert (np.count_nonzero(p["W1"], axis=0) == 1).all() and len(set(np.nonzero(p["W1"])[0])) == spec.hid
    assert set(p["src"]) == set(range(p["x"].shape[0]))
    ref = R.reference(spec, p["W1"], p["b1"], p["W2"], p["b2"], p["ea"], p["x"][p["src"]], p["sh"], form)
    bound = R.probe_bound(ref, form)
    assert (bound > 0)[ref.msg != 0].all() and np.count_nonzero(ref.msg) > 0.3 * ref.msg.size
    emu = R.emulate(spec, p["W1"], p["b1"], p["W2"], p["b2"], p["ea"], p["x"], p["src"], p["sh"], form)
    ratio = np.abs(emu - ref.msg) / np.maximum(bound, 1e-300)
    print(f"[emulated] probe {form} band {band}: max err/bound {ratio.max():.3f}")
    assert (np.abs(emu - ref.msg) <= bound).all(), ratio.max()
    if band[0] == -3.0:      # (lo halves normal but for the smallest G values: the floors are small beside the relative part)
        assert (ref.floor <= 0.25 * bound).all()


@pytest.mark.parametrize("form,mutation,kinds", [
    (R.Form("rows", True, 1), "drop_lo", None), (R.Form("rows", True, 0), "drop_lo", None), (R.Form("rows", False, 0), "drop_lo", None),
    (R.Form("h2", True, 0), "drop_lo", None),
    (R.Form("rows", True, 1), "ignore_byte", (R.F_SCALAR_S0, R.F_SCALAR_S1)),
    (R.Form("rows", True, 1), "w2_lo_scale", (R.F_DOT, R.F_VEC_S0, R.F_CROSS)),
    (R.Form("rows", False, 0), "w2_lo_scale", None)])
def test_probe_bound_rejects_a_lost_plane(form, mutation, kinds):
    """Three mutations of the emulated operands, each worth about 2^-12 of a term - lo planes dropped, G's continuation byte ignored, the
    lo plane of the fc.3 operand at 1 / 2048 of its scale: outside the probe bound on at least one element of every block they touch."""
    spec, p = _probe(-3.0, 3.0)
    ref = R.reference(spec, p["W1"], p["b1"], p["W2"], p["b2"], p["ea"], p["x"][p["src"]], p["sh"], form)
    bound = R.probe_bound(ref, form)
    emu = R.emulate(spec, p["W1"], p["b1"], p["W2"], p["b2"], p["ea"], p["x"], p["src"], p["sh"], form, mutate=mutation)
    out = np.abs(emu - ref.msg) > bound
    blocks = spec.blocks if kinds is None else _blocks_of(spec, kinds)
    assert blocks
    for b in blocks:
        cols = slice(b.out_off, b.out_off + b.n * b.C)
        assert out[:, cols].any(), (mutation, b.out_off)
    print(f"[emulated] {mutation} {form}: {int(out.sum())} of {out.size} elements outside the probe bound, "
          f"max err/bound {float((np.abs(emu - ref.msg) / np.maximum(bound, 1e-300)).max()):.1f}")


def _dense_case(E=500, N=40, ns=32, nv=6, layer=3, seed=2):
    mi, mo = P.irreps_muls(ns, nv, layer), P.irreps_muls(ns, nv, layer + 1)
    spec = P.faster_tp_spec(mi, mo, 3 * ns)
    sd = _fc(spec, seed)
    x, src, ea, sh = _inputs(spec, P.irreps_dim(mi), E, N, seed)
    src = torch.sort(src)[0]
    recv = torch.randint(0, N, (E,), generator=torch.Generator().manual_seed(seed + 1))
    f32 = lambda t: t.float().numpy()      # noqa: E731
    return spec, [f32(sd[k]) for k in ("c.fc.0.weight", "c.fc.0.bias", "c.fc.3.weight", "c.fc.3.bias")], f32(x), src.numpy(), f32(ea), f32(sh), recv


def _mean(msg, recv, N):
    return tp.scatter(torch.from_numpy(msg), recv, dim=0, dim_size=N, reduce="mean")


def test_dense_bound_rejects_a_near_duplicate_wrong_row_that_the_old_metric_accepts():
    """The premise that the old metric accepts a swapped edge at E = 500 does NOT hold for a genuine swap of two unrelated source rows: the
    old metric rejects that too (next test).  What it can miss is a wrong row whose error is of the operand planes' own size, once the mean
    runs over enough edges - the constructed case here.  One wrong message row in a 500-edge set.  Two edges read each other's source row (their `src` swapped in the emulation); the two source
    nodes' features differ by about 2^-12 of themselves - the size of a lost operand plane.  The element-wise dense bound rejects it; the
    metric that guarded the convs before - rel_err = max|diff| / max|ref| AFTER the segmented mean, < 2e-5
    (test_single_conv_layer) - accepts it once the mean runs over enough edges: asserted with the 500 edges on 4 receivers (125 per mean).
    On 40 receivers (12.5 per mean, test_single_conv_layer's own case) it reads 4.2e-5 and would still object: what the old metric
    cannot see depends on the degree, what the element-wise bound sees does not.  With the documented rounding alone, every element is
    inside the dense bound."""
    spec, (W1, b1, W2, b2), x, src, ea, sh, recv = _dense_case()
    form = R.Form("rows", True, 1)
    N = x.shape[0]
    e0 = int(np.argmax(src == 7))
    e1 = int(np.argmax(src == 8))
    x[8] = (x[7].astype(np.float64) * (1.0 + 2.0 ** -12 * np.sign(np.sin(np.arange(x.shape[1]) + 0.5)))).astype(np.float32)
    ref = R.reference(spec, W1, b1, W2, b2, ea, x[src], sh, form)
    good = R.emulate(spec, W1, b1, W2, b2, ea, x, src, sh, form)
    assert (np.abs(good - ref.msg) <= ref.bound).all(), float((np.abs(good - ref.msg) / ref.bound).max())
    bad = R.emulate(spec, W1, b1, W2, b2, ea, x, src, sh, form, swap=(e0, e1))
    out = np.abs(bad - ref.msg) > ref.bound
    assert out[e0].any() and out[e1].any() and not np.delete(out, [e0, e1], axis=0).any()
    old40 = rel_err(_mean(bad, recv, N), _mean(ref.msg, recv, N))
    old = rel_err(_mean(bad, recv % 4, 4), _mean(ref.msg, recv % 4, 4))
    print(f"[emulated] swapped rows: {int(out.sum())} elements outside the dense bound, max err/bound "
          f"{float((np.abs(bad - ref.msg) / ref.bound).max()):.1f}; rel_err after the mean: {old:.3e} on 4 receivers, {old40:.3e} on 40")
    assert old < 2e-5, old


def test_a_grossly_wrong_row_is_seen_by_both_metrics():
    """(For the record: two UNRELATED source rows swapped - an O(1) error in two of 500 rows - fail the old metric too; what it cannot
    see is an error of the operand planes' own size.)"""
    spec, (W1, b1, W2, b2), x, src, ea, sh, recv = _dense_case()
    form = R.Form("rows", True, 1)
    e0, e1 = int(np.argmax(src == 7)), int(np.argmax(src == 8))
    ref = R.reference(spec, W1, b1, W2, b2, ea, x[src], sh, form)
    bad = R.emulate(spec, W1, b1, W2, b2, ea, x, src, sh, form, swap=(e0, e1))
    assert (np.abs(bad - ref.msg) > ref.bound)[[e0, e1]].any(axis=1).all()
    assert rel_err(_mean(bad, recv, x.shape[0]), _mean(ref.msg, recv, x.shape[0])) > 2e-5


def test_plane_emulation_matches_the_packers():
    """The emulated roundings are the packers' own: packing.split_h2's planes (both forms) stand for the values split_unified / split_h2
    give, and plane form 1 keeps 19 significant bits (truncated hi word + byte), 11 without the byte."""
    g = torch.Generator().manual_seed(0)
    W = (torch.randn(1, 16, 8, generator=g) * torch.exp2(torch.randint(-12, 6, (1, 16, 8), generator=g).float()))
    for S in (0.0, P.GH_SW):
        pl = P.split_h2(W, unified_scale=S).double()                  # [1, 2, k/16, 2, ncols, 8]
        hi, lo = (pl[0, q].permute(0, 1, 3, 2).reshape(16, 8) for q in (0, 1))
        mine = R.split_unified(W[0].numpy(), S) if S else R.split_h2(W[0].numpy())
        want = ((hi + lo) / S if S else hi + lo / 2048.0).numpy()
        assert np.array_equal(mine, want)
    V = np.exp2(np.linspace(-13.9, 10, 4001)) * np.where(np.arange(4001) % 2, 1.0, -1.0) * 1.2345
    full, cut = R.g_plane_form1(V), R.g_plane_form1(V, ignore_byte=True)
    assert (np.abs(full - V) <= 2.0 ** -19 * np.abs(V)).all() and (np.abs(cut - V) <= 2.0 ** -10 * np.abs(V)).all()
    assert (np.abs(cut) <= np.abs(full)).all() and float((np.abs(cut - V) / np.abs(V)).max()) > 2.0 ** -11
    assert np.array_equal(cut, cut.astype(np.float16).astype(np.float64))
