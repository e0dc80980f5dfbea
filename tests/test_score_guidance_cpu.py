"""CPU tests of the physics-score guidance term (diffdock_pocket_amd/score_guidance.py, Sampler with score_guidance_weight > 0)
against the float64 restatement of tests/score_guidance_ref.py.  The PyTorch form and the restatement are both fp64 evaluations of
the same definition in other summation orders: they are held to score_guidance_ref.bounds (the fp64 summation bound of
vinardo_ref.bounds on energy and gradient, carried through the direction and the cap factor by guidance_ref.bounds, plus
4 2^-24 |increment| for the fp32 roundings).  Every case asserts the margins of score_guidance_ref.margins_ok before it compares."""
import dataclasses
import functools
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref as GR
import score_guidance_ref as R
import vinardo_ref as V
from diffdock_pocket_amd import guidance as G
from diffdock_pocket_amd import sampler as S
from diffdock_pocket_amd import score_guidance as SG
from diffdock_pocket_amd.diffusion import get_t_schedule
from diffdock_pocket_amd.scoring import ScoreConfig
from diffdock_pocket_amd.synthetic import make_3dpf_complex
from test_guidance_cpu import Stub

# (S, n, m, T, per-sample receptor, self pairs): the shapes the issue lists; tests/test_gpu_score_guidance.py adds the limit shape
SHAPES = [(1, 1, 0, 0, False, False), (3, 1, 1023, 0, False, False), (1, 4, 1, 1, False, True), (3, 5, 1024, 5, True, True),
          (4, 37, 1025, 7, True, True), (2, 256, 300, 0, False, True)]
LIMIT_SHAPE = (1, 1024, 2, 1024, False, False)
INF = float("inf")


def shape_id(s):
    return "S{}_n{}_m{}_T{}_{}_{}".format(*s)


@functools.lru_cache(maxsize=None)
def case(shape):
    """The random case of a shape, drawn once and shared (nobody writes into it)."""
    S_, n, m, T, per_sample, with_pairs = shape
    return R.random_case(S_, n, m, T, seed=1000 * n + m + T + S_, per_sample_rec=per_sample, with_pairs=with_pairs)


def case_tables(c, config=None):
    t = torch.from_numpy
    return SG.ScoreGuidanceTables(t(c["lig_r"]), t(c["lig_f"]), t(c["rec"]), t(c["rec_r"]), t(c["rec_f"]),
                                  t(c["pairs"]) if c["pairs"] is not None else None, t(c["bonds"]), t(c["mask"]), config or ScoreConfig())


# ---------------------------------------------------------------------------------------------- 1. the PyTorch form
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_pytorch_form_matches_the_restatement(shape):
    S_, n, m, T, per_sample, with_pairs = shape
    c = case(shape)
    ref = c["ref"]
    assert R.margins_ok(ref, n)
    tb = case_tables(c)
    x, rec = torch.from_numpy(c["x"]), torch.from_numpy(c["rec"])
    from diffdock_pocket_amd.minimize import energy_torch
    e, g = energy_torch(x, x, tb.lig_radii, tb.lig_flags, rec, tb.rec_radii, tb.rec_flags, tb.self_pairs, tb.config, 0.0)
    be, bg, bu = R.bounds(ref, n)
    err_e, err_g = np.abs(e[:, :2].numpy() - ref["eg"]["e"]), np.abs(g.numpy() - ref["eg"]["g"])
    print(f"[score guidance] {shape} torch form: energy err/bound {float((err_e / be).max()):.3e}, gradient err/bound "
          f"{float((err_g / bg[:, None, None]).max()):.3e}")
    assert bool((err_e <= be).all()) and bool((err_g <= bg[:, None, None]).all())
    assert bool((e[:, 2] == 0).all()) and torch.equal(e[:, 3], e[:, 0] + e[:, 1])       # restraint 0: E = inter + intra
    inc = SG.increments_torch(x, rec, tb, c["w"], c["caps"])
    for k, (got, want) in enumerate(zip(inc, ref["inc"])):
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        err = np.abs(got.numpy().astype(np.float64) - want.astype(np.float64))
        print(f"[score guidance] {shape} torch form: increment {k} err/bound {float((err / np.maximum(bu[k], 1e-300)).max(initial=0.0)):.3e}")
        assert bool((err <= bu[k]).all()), (shape, k)
    if S_ > 1 and (c["need"] > 0).sum() > 1:
        assert ref["capped"].any() and not ref["capped"].all()          # capped and uncapped samples in one case
    assert SG.increments_torch(x, rec, tb, 0.0, c["caps"]) is None and SG.increments_torch(x, rec, tb, -0.0, c["caps"]) is None


def test_the_limit_shape_keeps_its_margins():
    c = case(LIMIT_SHAPE)
    assert R.margins_ok(c["ref"], LIMIT_SHAPE[1])


# ---------------------------------------------------------------------------------------------- 2. the caps
def test_each_cap_binds_in_turn_and_none():
    caps = (1.0, 0.5, 0.5)
    # (direction, factor): translation of norm 2 -> 0.5; rotation of norm 2 -> 0.25; one torsion of 5 -> 0.1; all inside -> 1
    cases = [(([2.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.1, -0.2]), 0.5), (([0.0, 0.6, 0.8], [0.0, 2.0, 0.0], [0.1, -0.2]), 0.25),
             (([0.3, 0.0, 0.0], [0.1, 0.0, 0.0], [0.1, -5.0]), 0.1), (([0.6, 0.0, 0.8], [0.3, 0.0, 0.4], [0.5, -0.5]), 1.0),
             (([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0]), 1.0)]
    for (tr, rot, tor), want in cases:
        d = [torch.tensor([v], dtype=torch.float32) for v in (tr, rot, tor)]
        f = SG.cap_factor(d[0], d[1], d[2], *caps)
        fr, _ = GR.cap_factor([v.numpy() for v in d], caps)
        assert float(f) == pytest.approx(want, rel=1e-7) and float(fr[0]) == pytest.approx(want, rel=1e-7), (tr, rot, tor)
    assert SG.cap_factor is G.cap_factor                       # one cap rule for both guidance terms


# ---------------------------------------------------------------------------------------------- the CPU sampler
def _graph(flex):
    return make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=20) if flex else make_3dpf_complex(seed=0, flexible_sidechains=False)


def _sampler(cfg, flex=False, n=4, sl=None, seed=3):
    g = _graph(flex)
    T, n_sc = int(g["ligand"].edge_mask.sum()), (int(g["flexResidues"].edge_idx.shape[0]) if flex else 0)
    return S.Sampler(Stub(T, n_sc), g, n, torch.device("cpu"), dataclasses.replace(cfg, flexible_sidechains=flex), seed=seed, sample_slice=sl), g


GUIDED = S.SamplerConfig(inference_steps=3, no_random=True, score_guidance_weight=0.5)


# ---------------------------------------------------------------------------------------------- 3. off means off
@pytest.mark.parametrize("flex", [False, True])
def test_zero_weight_and_t_above_t_max_change_nothing(flex):
    outs = []
    for cfg in (S.SamplerConfig(inference_steps=3), S.SamplerConfig(inference_steps=3, score_guidance_weight=0.0, score_guidance_max_tr=0.1),
                S.SamplerConfig(inference_steps=3, score_guidance_weight=2.0, score_guidance_t_max=0.0)):
        smp, _ = _sampler(cfg, flex)
        assert smp.score_guidance == (cfg.score_guidance_weight > 0) and (smp.score_guidance or not hasattr(smp, "sguid_tables"))
        smp.randomize()
        outs.append(smp.run(get_t_schedule(3)))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    d = S.SamplerConfig()
    assert (d.score_guidance_weight, d.score_guidance_t_max, d.score_guidance_max_tr, d.score_guidance_max_rot,
            d.score_guidance_max_tor, d.score_guidance_config) == (0.0, 1.0, 1.0, 0.5, 0.5, None)
    assert SG.step_weight(0.5, 0.3, 0.3) == 0.5 and SG.step_weight(0.5, 0.31, 0.3) == 0.0


# ---------------------------------------------------------------------------------------------- 4. one guided step
def _ref_forward(tb, pos0, rec, w, caps, base):
    return R.forward(pos0, tb.lig_radii.numpy(), tb.lig_flags.numpy(), rec, tb.rec_radii.numpy(), tb.rec_flags.numpy(),
                     tb.self_pairs.numpy(), tb.bonds.numpy(), tb.mask_rotate.numpy(), w, caps, base)


def _unguided_updates(plain, flex, pos0, sched):
    """What the same step applies without the term, recovered from a sampler that records them."""
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
    return seen["upd"], ref_smp


@pytest.mark.parametrize("flex,no_torsion,ode", [(False, False, False), (True, False, False), (False, True, False), (True, True, False),
                                                 (False, False, True), (True, False, True), (False, True, True), (True, True, True)])
def test_one_guided_step_is_the_unguided_update_plus_the_restatement(flex, no_torsion, ode):
    cfg = dataclasses.replace(GUIDED, no_torsion=no_torsion, ode=ode, score_guidance_max_tr=0.4)
    sched = get_t_schedule(3)
    smp, g = _sampler(cfg, flex)
    smp.randomize()
    pos0, apos0 = smp.lig_pos.clone(), smp.atom_pos.clone()
    tb = smp.sguid_tables
    T = int(tb.bonds.shape[0])
    assert T == (0 if no_torsion else smp.T)
    base, ref_smp = _unguided_updates(dataclasses.replace(cfg, score_guidance_weight=0.0), flex, pos0, sched)
    rec = apos0.numpy() if flex else tb.rec.numpy()
    want = _ref_forward(tb, pos0.numpy(), rec, cfg.score_guidance_weight, (0.4, 0.5, 0.5),
                        [base[0].numpy(), base[1].numpy(), base[2].numpy() if base[2] is not None else np.zeros((4, 0), np.float32)])
    assert R.margins_ok(want, smp.n_l)
    assert max(float(np.abs(i).max(initial=0.0)) for i in want["inc"]) > 1e-3          # the term did contribute
    upd = [torch.from_numpy(u) for u in want["upd"]]
    expect = S.modify_conformer(pos0, upd[0], upd[1], upd[2] if base[2] is not None else None, smp.bonds, smp.rot_idx)
    smp.step(0, sched)
    d = float((smp.lig_pos - expect).abs().max())
    print(f"[score guidance] cpu step flex={flex} no_torsion={no_torsion} ode={ode}: poses differ by {d:.3e} A, capped "
          f"{want['capped'].tolist()}, moved {float((expect - ref_smp.lig_pos).abs().max()):.3f} A beyond the unguided step")
    assert d < 1e-5                                       # the same fp32 pose update on increments equal to one rounding
    assert torch.equal(smp.atom_pos, ref_smp.atom_pos)    # side chains get no guidance
    assert float((expect - ref_smp.lig_pos).abs().max()) > 1e-3


@pytest.mark.parametrize("flex", [False, True])
def test_with_clash_guidance_the_increments_add_in_order(flex):
    """unguided + clash increment + score increment, in that order of fp32 additions."""
    cfg = dataclasses.replace(GUIDED, clash_guidance_weight=0.5, clash_guidance_max_tr=0.3, score_guidance_max_tr=0.4)
    sched = get_t_schedule(3)
    smp, g = _sampler(cfg, flex)
    smp.randomize()
    pos0, apos0 = smp.lig_pos.clone(), smp.atom_pos.clone()
    base, ref_smp = _unguided_updates(dataclasses.replace(cfg, score_guidance_weight=0.0, clash_guidance_weight=0.0), flex, pos0, sched)
    base = [b.numpy() for b in base]
    ct, tb = smp.guid_tables, smp.sguid_tables
    clash = GR.forward(pos0.numpy(), ct.lig_radii.numpy(), apos0.numpy() if flex else ct.rec.numpy(), ct.rec_radii.numpy(), ct.self_pairs.numpy(),
                       ct.bonds.numpy(), ct.mask_rotate.numpy(), 0.5, (0.3, 0.5, 0.5), base)
    assert GR.margins_ok(clash, smp.n_l)
    want = _ref_forward(tb, pos0.numpy(), apos0.numpy() if flex else tb.rec.numpy(), 0.5, (0.4, 0.5, 0.5), clash["upd"])
    assert R.margins_ok(want, smp.n_l)
    assert max(float(np.abs(i).max()) for i in clash["inc"]) > 1e-3 and max(float(np.abs(i).max()) for i in want["inc"]) > 1e-3
    upd = [torch.from_numpy(u) for u in want["upd"]]
    expect = S.modify_conformer(pos0, upd[0], upd[1], upd[2], smp.bonds, smp.rot_idx)
    smp.step(0, sched)
    d = float((smp.lig_pos - expect).abs().max())
    print(f"[score guidance] cpu step with clash guidance flex={flex}: poses differ by {d:.3e} A")
    assert d < 1e-5
    # the sum is ordered: the torch forms' own increments, added in the definition's order, give the step's poses bit for bit
    ci = G.increments_torch(pos0, apos0 if flex else ct.rec, ct, 0.5, 0.3, 0.5, 0.5)
    si = SG.increments_torch(pos0, apos0 if flex else tb.rec, tb, 0.5, (0.4, 0.5, 0.5))
    exact = [(torch.from_numpy(b) + c) + s for b, c, s in zip(base, ci, si)]
    assert torch.equal(S.modify_conformer(pos0, exact[0], exact[1], exact[2], smp.bonds, smp.rot_idx), smp.lig_pos)


# ---------------------------------------------------------------------------------------------- 5. slices
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


# ---------------------------------------------------------------------------------------------- 6. descent on the 3dpf fixture
DESCENT_SHIFT = (1.5, 0.0, 0.0)
DESCENT_WEIGHT = 1.0          # halved from 1 until the restatement shows a decrease: see the test


def test_one_increment_descends_on_the_shifted_crystal_pose():
    """Only the guidance increments of one step, with infinite caps, applied to the crystal pose of the 3dpf fixture translated by
    1.5 A.  DESCENT_WEIGHT was fixed by halving from 1 until the restatement's E falls; the restatement's figures at the weights
    tried are printed.  E falls and the translation increment points back."""
    from test_evaluation_cpu import graph_3dpf
    g, _ = graph_3dpf()
    tb = SG.build_tables(g)
    shift = np.array(DESCENT_SHIFT, np.float32)
    x0 = (g["ligand"].pos.float().numpy() + shift)[None]
    rot_idx = S.rotate_index_lists(tb.mask_rotate)

    def energy(x):
        sc = V.score(x, tb.lig_radii.numpy(), tb.lig_flags.numpy(), tb.rec.numpy(), tb.rec_radii.numpy(), tb.rec_flags.numpy(),
                     tb.self_pairs.numpy())
        return float(sc["energy"][0, 4] + sc["energy"][0, 5])

    def moved(w):
        ref = _ref_forward(tb, x0, tb.rec.numpy(), w, (INF, INF, INF), None)
        inc = [torch.from_numpy(i) for i in ref["inc"]]
        return ref, S.modify_conformer(torch.from_numpy(x0), inc[0], inc[1], inc[2], tb.bonds, rot_idx).numpy()

    e0 = energy(x0)
    w = 1.0
    while True:                                                 # the rule that fixed DESCENT_WEIGHT, run again on the restatement
        ref, x1 = moved(w)
        e1 = energy(x1)
        print(f"[score guidance] descent: w = {w}: E {e0:.4f} -> {e1:.4f}, |inc_tr| {float(np.linalg.norm(ref['inc'][0])):.4f} A")
        if e1 < e0 or w < 1e-6:
            break
        w *= 0.5
    assert w == DESCENT_WEIGHT
    assert R.margins_ok(ref, tb.n)
    assert e1 < e0
    assert float(ref["inc"][0][0].astype(np.float64) @ (-shift.astype(np.float64))) > 0
    # the package's own form takes the same step
    inc = SG.increments_torch(torch.from_numpy(x0), tb.rec, tb, DESCENT_WEIGHT, (INF, INF, INF))
    x1p = S.modify_conformer(torch.from_numpy(x0), inc[0], inc[1], inc[2], tb.bonds, rot_idx).numpy()
    assert energy(x1p) < e0 and float(inc[0][0].double().numpy() @ (-shift.astype(np.float64))) > 0
    assert float(np.abs(x1p - x1).max()) < 1e-5


# ---------------------------------------------------------------------------------------------- 7. - 10. configuration and ABI
FIELDS = ("score_guidance_weight", "score_guidance_t_max", "score_guidance_max_tr", "score_guidance_max_rot", "score_guidance_max_tor")


def test_config_validation():
    for field in FIELDS:
        for bad in (-0.1, float("nan")):
            with pytest.raises(ValueError, match=field):
                S.SamplerConfig(**{field: bad})
    with pytest.raises(ValueError, match="finite"):
        S.SamplerConfig(score_guidance_weight=float("inf"))
    S.SamplerConfig(score_guidance_weight=1.0, score_guidance_max_tr=float("inf"))          # no cap
    with pytest.raises(ValueError, match="score_guidance_weight"):
        dataclasses.replace(S.SamplerConfig(), score_guidance_weight=-1.0)
    with pytest.raises(ValueError, match="cutoff"):
        S.SamplerConfig(score_guidance_weight=1.0, score_guidance_config=ScoreConfig(cutoff=-1.0))
    with pytest.raises(ValueError, match="score_guidance_max_rot"):
        G.check_config(1.0, 1.0, 1.0, -1.0, 1.0, prefix="score_guidance")
    # the form's constants reach the term
    smp, _ = _sampler(dataclasses.replace(GUIDED, score_guidance_config=ScoreConfig(cutoff=6.0)))
    assert smp.sguid_tables.config.cutoff == 6.0


def test_a_ligand_above_the_kernel_limit_raises_at_construction():
    g = _graph(False)
    for name, limit in (("MAX_ATOMS", 36), ("MAX_TORSIONS", 4)):      # the synthetic 3dpf ligand: 37 atoms, 5 rotatable bonds
        old = getattr(SG, name)
        setattr(SG, name, limit)
        try:
            with pytest.raises(ValueError, match="exceeds the limits"):
                S.Sampler(Stub(5, 0), g, 2, torch.device("cpu"), GUIDED)
            S.Sampler(Stub(5, 0), g, 2, torch.device("cpu"), S.SamplerConfig())               # unguided: not looked at
        finally:
            setattr(SG, name, old)
    assert SG.MAX_ATOMS == 1024 and SG.MAX_TORSIONS == 1024


def test_command_line_flags_reach_the_sampler_config():
    from diffdock_pocket_amd.inference import _guidance_fields, _parser
    d = _parser().parse_args([])
    assert (d.score_guidance, d.score_guidance_t_max, d.score_guidance_max_tr, d.score_guidance_max_rot, d.score_guidance_max_tor) == \
        (0.0, 1.0, 1.0, 0.5, 0.5)
    assert S.SamplerConfig(**_guidance_fields(d)) == S.SamplerConfig()
    a = _parser().parse_args(["--score_guidance", "0.75", "--score_guidance_t_max", "0.4", "--score_guidance_max_tr", "2",
                              "--score_guidance_max_rot", "0.25", "--score_guidance_max_tor", "0.125", "--clash_guidance", "0.5"])
    cfg = S.SamplerConfig(**_guidance_fields(a))
    assert tuple(getattr(cfg, f) for f in FIELDS) == (0.75, 0.4, 2.0, 0.25, 0.125)
    assert cfg.clash_guidance_weight == 0.5 and cfg.clash_guidance_max_tr == 1.0


def test_c_abi_declares_the_score_guidance_entry():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import build as B
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ddp_hip.h")).read()
    assert re.findall(r"^int\s+(ddp_score_guidance)\s*\(", header, flags=re.M) == ["ddp_score_guidance"]
    assert "ddp_score_guidance" in L.EXPORTS and "ddp_score_guidance.hip" in B.SOURCES
    assert "#define DDP_ABI_VERSION 17" in header
    assert L.DDP_GUIDANCE_MAX_TORSIONS == SG.MAX_TORSIONS == 1024 and L.DDP_EVAL_MAX_ATOMS == SG.MAX_ATOMS
    # the ctypes struct follows the header's field order
    end = header.index("} ddp_score_guidance_args_t;")
    body = header[header.rindex("typedef struct {", 0, end):end]
    names = re.findall(r"[\s\*]([a-z_]+)(?:\[3\])?[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in L.ScoreGuidanceArgs._fields_]
    assert L.ScoreGuidanceArgs.form.size == L.ScoreArgs.form.size == 11 * 8
