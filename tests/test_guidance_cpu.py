"""CPU tests of the steric-clash guidance term (diffdock_pocket_amd/guidance.py, Sampler with clash_guidance_weight > 0) against the
float64 restatement of tests/guidance_ref.py.  The PyTorch form and the restatement are both fp64 evaluations of the same definition
in other summation orders: rtol 1e-9 on the unrounded quantities, and the fp32 increments may differ by one rounding of an fp64 value
that sits on a rounding boundary (2^-23 relative).  Every case asserts the margins of guidance_ref.margins_ok before it compares."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref as R
from diffdock_pocket_amd import guidance as G
from diffdock_pocket_amd import sampler as S
from diffdock_pocket_amd.diffusion import get_t_schedule
from diffdock_pocket_amd.synthetic import make_3dpf_complex

# (S, n, m, T, per-sample receptor, self pairs): the shapes of the kernel test of tests/test_gpu_guidance.py
SHAPES = [(1, 1, 0, 0, False, False), (3, 1, 1023, 0, False, False), (1, 4, 1, 1, False, True), (3, 5, 1024, 5, True, True),
          (3, 37, 1025, 5, False, True), (1, 37, 0, 5, False, True), (3, 37, 2 * 1024 + 37, 1, True, False), (3, 256, 1, 5, False, True),
          (1, 256, 1023, 0, True, True), (3, 1024, 1025, 5, False, True), (1, 1024, 2 * 1024 + 37, 1, True, False),
          (3, 4, 1024, 0, True, True), (1, 5, 1025, 1, False, False)]


def case_tables(c):
    t = torch.from_numpy
    return G.GuidanceTables(t(c["lig_r"]), t(c["rec"]), t(c["rec_r"]), t(c["pairs"]) if c["pairs"] is not None else None,
                            t(c["bonds"]), t(c["mask"]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "S{}_n{}_m{}_T{}_{}_{}".format(*s))
def test_pytorch_form_matches_the_restatement(shape):
    S_, n, m, T, per_sample, with_pairs = shape
    c = R.random_case(S_, n, m, T, seed=1000 * n + m + T + S_, per_sample_rec=per_sample, with_pairs=with_pairs)
    ref = c["ref"]
    assert R.margins_ok(ref, n)
    tb = case_tables(c)
    x, rec = torch.from_numpy(c["x"]), torch.from_numpy(c["rec"])
    from diffdock_pocket_amd.descent import direction_torch
    from diffdock_pocket_amd.refine import energy_torch
    e, g = energy_torch(x, x, tb.lig_radii, rec, tb.rec_radii, tb.self_pairs, R.OVERLAP, 0.0)
    np.testing.assert_allclose(e[:, :2].numpy(), ref["eg"]["e"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(g.numpy(), ref["eg"]["g"], rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(ref["eg"]["g"]).max())))
    d = direction_torch(x, g, tb.bonds, tb.mask_rotate)
    for got, key in zip(d, ("d_tr", "d_rot", "d_tor")):
        np.testing.assert_allclose(got.numpy(), ref["dr"][key], rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(ref["dr"][key]).max(initial=0.0))))
    inc = G.increments_torch(x, rec, tb, c["w"], *c["caps"])
    f = G.cap_factor(*[torch.from_numpy(v) for v in ref["d32"]], *c["caps"])
    np.testing.assert_allclose(f.numpy(), ref["f"], rtol=1e-9)
    for got, want in zip(inc, ref["inc"]):
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        # (atol: a component that cancels exactly in exact arithmetic - the net force of the ligand's own pairs - is rounding noise)
        np.testing.assert_allclose(got.numpy(), want, rtol=2.0 ** -22, atol=1e-9 * max(1.0, float(np.abs(want).max(initial=0.0))))
    if S_ > 1 and (c["need"] > 0).sum() > 1 and c["need"].max() > c["need"][c["need"] > 0].min():
        assert ref["capped"].any() and not ref["capped"].all()


def _hand_case(d_tr, d_rot, d_tor):
    return [torch.tensor([v], dtype=torch.float32) for v in (d_tr, d_rot, d_tor)]


def test_each_cap_binds_in_turn_and_none():
    caps = (1.0, 0.5, 0.5)
    # (direction, factor): translation of norm 2 -> 0.5; rotation of norm 2 -> 0.25; one torsion of 5 -> 0.1; all inside -> 1
    cases = [(([2.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.1, -0.2]), 0.5), (([0.0, 0.6, 0.8], [0.0, 2.0, 0.0], [0.1, -0.2]), 0.25),
             (([0.3, 0.0, 0.0], [0.1, 0.0, 0.0], [0.1, -5.0]), 0.1), (([0.6, 0.0, 0.8], [0.3, 0.0, 0.4], [0.5, -0.5]), 1.0),
             (([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0]), 1.0)]
    for (tr, rot, tor), want in cases:
        d = _hand_case(tr, rot, tor)
        f = G.cap_factor(d[0], d[1], d[2], *caps)
        fr, _ = R.cap_factor([v.numpy() for v in d], caps)
        assert float(f) == pytest.approx(want, rel=1e-7) and float(fr[0]) == pytest.approx(want, rel=1e-7), (tr, rot, tor)
    # no torsions; caps of +infinity never bind; a cap of 0 stops the move
    d = _hand_case([3.0, 0.0, 4.0], [0.0, 0.0, 0.1], [])
    assert float(G.cap_factor(d[0], d[1], d[2].reshape(1, 0), *caps)) == pytest.approx(0.2)
    assert float(G.cap_factor(d[0], d[1], None, float("inf"), float("inf"), float("inf"))) == 1.0
    assert float(G.cap_factor(d[0], d[1], None, 0.0, 0.5, 0.5)) == 0.0


class Stub:
    """A deterministic stand-in for the score model: a pure function of the positions."""

    def __init__(self, T, n_sc):
        self.T, self.n_sc = T, n_sc

    def __call__(self, b):
        B = b.num_graphs
        lp, ap = b["ligand"].pos.reshape(B, -1, 3), b["atom"].pos.reshape(B, -1, 3)
        c = lp.mean(1)
        return (-0.05 * c + 0.01 * lp[:, 0], 0.02 * torch.stack([c[:, 1], -c[:, 0], c[:, 2]], 1),
                0.01 * lp[:, :self.T, 0].reshape(-1) - 0.02, 0.01 * ap[:, :self.n_sc, 1].reshape(-1) + 0.015)


def _graph(flex):
    return make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=20) if flex else make_3dpf_complex(seed=0, flexible_sidechains=False)


def _sampler(cfg, flex=False, n=4, sl=None, seed=3):
    g = _graph(flex)
    T, n_sc = int(g["ligand"].edge_mask.sum()), (int(g["flexResidues"].edge_idx.shape[0]) if flex else 0)
    return S.Sampler(Stub(T, n_sc), g, n, torch.device("cpu"), dataclasses.replace(cfg, flexible_sidechains=flex), seed=seed, sample_slice=sl), g


GUIDED = S.SamplerConfig(inference_steps=3, no_random=True, clash_guidance_weight=0.5)


@pytest.mark.parametrize("flex", [False, True])
def test_zero_weight_and_t_above_t_max_change_nothing(flex):
    outs = []
    for cfg in (S.SamplerConfig(inference_steps=3), S.SamplerConfig(inference_steps=3, clash_guidance_weight=0.0, clash_guidance_max_tr=0.1),
                S.SamplerConfig(inference_steps=3, clash_guidance_weight=2.0, clash_guidance_t_max=0.0)):
        smp, _ = _sampler(cfg, flex)
        assert smp.guidance == (cfg.clash_guidance_weight > 0) and (smp.guidance or not hasattr(smp, "guid_tables"))
        smp.randomize()
        outs.append(smp.run(get_t_schedule(3)))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    d = S.SamplerConfig()
    assert (d.clash_guidance_weight, d.clash_guidance_t_max, d.clash_guidance_max_tr, d.clash_guidance_max_rot,
            d.clash_guidance_max_tor) == (0.0, 1.0, 1.0, 0.5, 0.5)
    assert G.step_weight(0.5, 0.3, 0.3) == 0.5 and G.step_weight(0.5, 0.31, 0.3) == 0.0


@pytest.mark.parametrize("flex", [False, True])
def test_sliced_samplers_equal_the_whole_sampler(flex):
    sched = get_t_schedule(3)
    whole, _ = _sampler(GUIDED, flex)
    whole.randomize()
    lw, aw = whole.run(sched)
    parts = []
    for sl in (slice(0, 2), slice(2, 4)):
        p, _ = _sampler(GUIDED, flex, sl=sl)
        p.randomize()
        parts.append(p.run(sched))
    assert torch.equal(torch.cat([p[0] for p in parts]), lw) and torch.equal(torch.cat([p[1] for p in parts]), aw)
    unguided, _ = _sampler(S.SamplerConfig(inference_steps=3, no_random=True), flex)
    unguided.randomize()
    assert not torch.equal(unguided.run(sched)[0], lw)                 # the term did move the poses


@pytest.mark.parametrize("flex,no_torsion,ode", [(False, False, False), (True, False, False), (False, True, False), (True, False, True)])
def test_one_guided_step_is_the_unguided_update_plus_the_restatement(flex, no_torsion, ode):
    cfg = dataclasses.replace(GUIDED, no_torsion=no_torsion, ode=ode, clash_guidance_max_tr=0.4)
    plain = dataclasses.replace(cfg, clash_guidance_weight=0.0)
    sched = get_t_schedule(3)
    smp, g = _sampler(cfg, flex)
    smp.randomize()
    pos0, apos0 = smp.lig_pos.clone(), smp.atom_pos.clone()
    tb = smp.guid_tables
    T = int(tb.bonds.shape[0])
    assert T == (0 if no_torsion else smp.T)
    # the unguided updates: what the same step applies without the term, recovered from a sampler that records them
    seen = {}
    orig = S.modify_conformer

    def spy(pos, tr, rot, tor, bonds, mask):
        seen["upd"] = (tr.clone(), rot.clone(), None if tor is None else tor.clone())
        return orig(pos, tr, rot, tor, bonds, mask)

    ref_smp, _ = _sampler(plain, flex)
    ref_smp.randomize()
    assert torch.equal(ref_smp.lig_pos, pos0)
    S.modify_conformer = spy
    try:
        ref_smp.step(0, sched)
    finally:
        S.modify_conformer = orig
    base = seen["upd"]
    rec = apos0.numpy() if flex else tb.rec.numpy()
    want = R.forward(pos0.numpy(), tb.lig_radii.numpy(), rec, tb.rec_radii.numpy(), tb.self_pairs.numpy(), tb.bonds.numpy(),
                     tb.mask_rotate.numpy(), cfg.clash_guidance_weight, (0.4, 0.5, 0.5),
                     [base[0].numpy(), base[1].numpy(), base[2].numpy() if base[2] is not None else np.zeros((4, 0), np.float32)])
    assert R.margins_ok(want, smp.n_l)
    assert max(float(np.abs(i).max(initial=0.0)) for i in want["inc"]) > 1e-3          # the term did contribute
    upd = [torch.from_numpy(u) for u in want["upd"]]
    expect = S.modify_conformer(pos0, upd[0], upd[1], upd[2] if base[2] is not None else None, smp.bonds, smp.rot_idx)
    smp.step(0, sched)
    d = float((smp.lig_pos - expect).abs().max())
    print(f"[guidance] cpu step flex={flex} no_torsion={no_torsion} ode={ode}: poses differ by {d:.3e} A, capped {want['capped'].tolist()}, "
          f"moved {float((expect - ref_smp.lig_pos).abs().max()):.3f} A beyond the unguided step")
    assert d < 1e-5                                       # the same fp32 pose update on increments equal to one rounding
    assert torch.equal(smp.atom_pos, ref_smp.atom_pos)    # side chains get no guidance
    assert float((expect - ref_smp.lig_pos).abs().max()) > 1e-3


def test_config_validation():
    for field in ("clash_guidance_weight", "clash_guidance_t_max", "clash_guidance_max_tr", "clash_guidance_max_rot", "clash_guidance_max_tor"):
        for bad in (-0.1, float("nan")):
            with pytest.raises(ValueError, match=field):
                S.SamplerConfig(**{field: bad})
    with pytest.raises(ValueError, match="finite"):
        S.SamplerConfig(clash_guidance_weight=float("inf"))
    S.SamplerConfig(clash_guidance_weight=1.0, clash_guidance_max_tr=float("inf"))          # no cap
    with pytest.raises(ValueError, match="clash_guidance_weight"):
        dataclasses.replace(S.SamplerConfig(), clash_guidance_weight=-1.0)


def test_a_ligand_above_the_kernel_limit_raises_at_construction():
    g = _graph(False)
    old = G.MAX_ATOMS
    G.MAX_ATOMS = 36            # the 3dpf ligand has 37 atoms
    try:
        with pytest.raises(ValueError, match="exceeds the limits"):
            S.Sampler(Stub(5, 0), g, 2, torch.device("cpu"), GUIDED)
        S.Sampler(Stub(5, 0), g, 2, torch.device("cpu"), S.SamplerConfig())               # unguided: not looked at
    finally:
        G.MAX_ATOMS = old


def test_command_line_flags_reach_the_sampler_config():
    from diffdock_pocket_amd.inference import _guidance_fields, _parser
    d = _parser().parse_args([])
    assert (d.clash_guidance, d.clash_guidance_t_max, d.clash_guidance_max_tr, d.clash_guidance_max_rot, d.clash_guidance_max_tor) == \
        (0.0, 1.0, 1.0, 0.5, 0.5)
    assert S.SamplerConfig(**_guidance_fields(d)) == S.SamplerConfig()
    a = _parser().parse_args(["--clash_guidance", "0.75", "--clash_guidance_t_max", "0.4", "--clash_guidance_max_tr", "2",
                              "--clash_guidance_max_rot", "0.25", "--clash_guidance_max_tor", "0.125"])
    cfg = S.SamplerConfig(**_guidance_fields(a))
    assert (cfg.clash_guidance_weight, cfg.clash_guidance_t_max, cfg.clash_guidance_max_tr, cfg.clash_guidance_max_rot,
            cfg.clash_guidance_max_tor) == (0.75, 0.4, 2.0, 0.25, 0.125)


def test_c_abi_declares_the_guidance_entry():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import build as B
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ddp_hip.h")).read()
    assert re.findall(r"^int\s+(ddp_clash_guidance)\s*\(", header, flags=re.M) == ["ddp_clash_guidance"]
    assert "ddp_clash_guidance" in L.EXPORTS and "ddp_guidance.hip" in B.SOURCES
    assert "#define DDP_ABI_VERSION 17" in header and "#define DDP_GUIDANCE_MAX_TORSIONS 1024" in header
    assert L.DDP_GUIDANCE_MAX_TORSIONS == G.MAX_TORSIONS == 1024 and L.DDP_EVAL_MAX_ATOMS == G.MAX_ATOMS
    # the ctypes struct follows the header's field order
    body = header[header.index("#define DDP_GUIDANCE_MAX_TORSIONS"):header.index("} ddp_clash_guidance_args_t;")]
    names = re.findall(r"[\s\*]([a-z_]+)(?:\[3\])?[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in L.GuidanceArgs._fields_]
