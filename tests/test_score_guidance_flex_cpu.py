"""CPU tests of the side-chain part of the physics-score guidance term (diffdock_pocket_amd/score_guidance.py, steps S1 - S4; Sampler
with score_guidance_sidechains) against the float64 restatement of tests/score_guidance_flex_ref.py.  The PyTorch form and the
restatement are both fp64 evaluations of the same definition in other summation orders: they are held to
score_guidance_flex_ref.bounds (the fp64 summation bound bgy of flexmin_ref.bounds, carried through num / den and the cap factor,
plus 4 2^-24 |increment| for the fp32 roundings).  Every case asserts the margins of score_guidance_flex_ref.margins_ok first."""
import dataclasses
import functools
import os
import re

import numpy as np
import pytest
import torch

import flexmin_ref as F
import score_guidance_flex_ref as R
from diffdock_pocket_amd import minimize_flex as MF
from diffdock_pocket_amd import sampler as S
from diffdock_pocket_amd import score_guidance as SG
from diffdock_pocket_amd.diffusion import get_t_schedule
from diffdock_pocket_amd.scoring import ScoreConfig
from diffdock_pocket_amd.synthetic import make_3dpf_complex
from test_guidance_cpu import Stub

# (S, n, m, n_mov, n_sc): the smallest case; no side chains; fewer bonds than waves, bonds sharing atoms; the receptor crosses one LDS
# tile of 1024; the real 3dpf flexible counts, two tiles; both side-chain limits
SHAPES = [(1, 1, 3, 1, 1), (2, 5, 40, 0, 0), (3, 5, 64, 7, 3), (2, 37, 1025, 37, 17), (2, 12, 1100, 130, 68), (1, 64, 300, 256, 256)]
UNTYPED = (3, 5, 64, 7, 3, "untyped_moving")
CASES = SHAPES + [UNTYPED]


def shape_id(s):
    return "S{}_n{}_m{}_mov{}_sc{}".format(*s[:5]) + ("_untyped" if len(s) > 5 else "")


@functools.lru_cache(maxsize=None)
def case(shape):
    """The random case of a shape, drawn once and shared (nobody writes into it)."""
    return R.random_case(*shape[:5], seed=11 * sum(shape[:5]) + (1 if len(shape) > 5 else 0), untyped_moving=len(shape) > 5)


def case_tables(c, config=None):
    """(ScoreGuidanceTables, SidechainTables) of a case; the shared receptor of the ligand tables is sample 0's (not read by the
    flexible forms, which take each sample's own)."""
    t = torch.from_numpy
    tb = SG.ScoreGuidanceTables(t(c["lig_r"]), t(c["lig_f"]), t(c["y"][0].copy()), t(c["rec_r"]), t(c["rec_f"]),
                                t(c["pairs"]) if c["pairs"] is not None else None, t(c["bonds"]), t(c["mask"]), config or ScoreConfig())
    sc = MF.SidechainTables(t(c["mov"]), t(c["edge"]), t(c["sub"]), t(c["mapping"]), t(c["sc_pairs"]))
    return tb, sc


# ---------------------------------------------------------------------------------------------- 1. the PyTorch form
@pytest.mark.parametrize("shape", CASES, ids=shape_id)
def test_pytorch_form_matches_the_restatement(shape):
    S_, n, m, n_mov, n_sc = shape[:5]
    c = case(shape)
    ref = c["sg"]
    assert R.margins_ok(ref)
    if len(shape) > 5:
        assert c["rec_r"][c["mov"][0]] < 0                                # the untyped moving atom is there
    if S_ > 1 and n_sc and (c["need"] > 0).sum() > 1:
        assert ref["capped"].any() and not ref["capped"].all()            # capped and uncapped samples in one case
    tb, sc = case_tables(c)
    x, y = torch.from_numpy(c["x"]), torch.from_numpy(c["y"])
    inc = SG.increments_sc_torch(x, y, tb, sc, c["w"], c["max_sc"])
    assert inc.dtype == torch.float32 and tuple(inc.shape) == (S_, n_sc)
    bu = R.bounds(ref)
    err = np.abs(inc.numpy().astype(np.float64) - ref["inc"].astype(np.float64))
    print(f"[score guidance sc] {shape} torch form: err/bound {float((err / np.maximum(bu, 1e-300)).max(initial=0.0)):.3e}, largest "
          f"|increment| {float(np.abs(ref['inc']).max(initial=0.0)):.3e}, capped {ref['capped'].tolist()}")
    assert bool((err <= bu).all())
    assert SG.increments_sc_torch(x, y, tb, sc, 0.0, 0.5) is None and SG.increments_sc_torch(x, y, tb, sc, -0.0, 0.5) is None


def test_the_cases_hold_capped_and_uncapped_samples():
    seen = [case(s)["sg"]["capped"] for s in SHAPES if s[0] > 1 and s[4] > 0]
    assert len(seen) == 3 and all(c.any() and not c.all() for c in seen)


# ---------------------------------------------------------------------------------------------- 2. descent
def test_the_side_chain_increment_alone_descends():
    """Only the side-chain increment, applied through flexmin_ref.apply_sidechains: the restatement's inter + sc falls strictly for
    every sample with a non-zero d_sc.  The weight is small enough that no atom moves a tenth of the kink gap, so no pair crosses a
    kink or the cutoff on the way and E is smooth along the step."""
    gap = 1e-3
    c = F.random_case(2, 5, 30, 6, 3, seed=5, kink_gap=gap)
    c.update(bonds=np.zeros((0, 2), np.int64), mask=np.zeros((0, 5), bool))
    unit = R.forward(c, 1.0, np.inf)
    assert R.margins_ok(unit, gap)
    # |dy_a| <= sum_j |angle_j| * (largest distance of a moving atom from an axis point): a weight that keeps that below gap / 10
    reach = max(float(np.linalg.norm(c["y"][s, a] - c["y"][s, int(v)])) for s in range(2) for a in c["mov"] for _, v in c["edge"])
    w = float(np.float32(0.05 * gap / (reach * np.abs(unit["dr"]["d"]).sum(1).max())))
    ref = R.forward(c, w, np.inf)
    e0 = ref["fm"]["energy"]
    moved_any = False
    for s in range(2):
        y1 = F.apply_sidechains(c["y"][s], c["edge"], c["sub"], c["mapping"], ref["inc"][s].astype(np.float64))
        moved = float(np.abs(y1 - c["y"][s].astype(np.float64)).max())
        assert moved <= gap / 10
        c1 = dict(c, y=np.stack([y1 if k == s else c["y"][k].astype(np.float64) for k in range(2)]))
        e1 = F.energy(c1["x"], c1["y"], c1["x"], c1["y"], c["lig_r"], c["lig_f"], c["rec_r"], c["rec_f"], c["pairs"], c["mov"], c["sc_pairs"])["energy"]
        print(f"[score guidance sc] descent sample {s}: inter + sc {e0[s, 0] + e0[s, 2]:.12f} -> {e1[s, 0] + e1[s, 2]:.12f}, moved {moved:.3e} A")
        if np.abs(ref["d32"][s]).max() > 0:
            moved_any = True
            assert e1[s, 0] + e1[s, 2] < e0[s, 0] + e0[s, 2]
    assert moved_any


# ---------------------------------------------------------------------------------------------- 3. the cap
def test_the_cap_binds_and_does_not_bind():
    d = torch.tensor([[0.1, -2.0, 0.5], [0.1, -0.2, 0.3], [0.0, 0.0, 0.0]], dtype=torch.float32)
    f = SG.cap_factor_sc(d, 0.5)
    fr, mx = R.cap_factor(d.numpy(), 0.5)
    assert f.dtype == torch.float64 and f.tolist() == pytest.approx([0.25, 1.0, 1.0], rel=1e-7) and fr.tolist() == pytest.approx(f.tolist(), rel=1e-15)
    assert SG.cap_factor_sc(d, float("inf")).tolist() == [1.0, 1.0, 1.0]
    assert SG.cap_factor_sc(d[:, :0], 0.5).tolist() == [1.0, 1.0, 1.0]
    c = case(SHAPES[2])
    tb, sc = case_tables(c)
    x, y = torch.from_numpy(c["x"]), torch.from_numpy(c["y"])
    free = SG.increments_sc_torch(x, y, tb, sc, c["w"], float("inf"))
    capped = SG.increments_sc_torch(x, y, tb, sc, c["w"], c["max_sc"])
    for s, is_capped in enumerate(c["sg"]["capped"]):
        assert float(capped[s].abs().max()) == pytest.approx(0.5, rel=1e-6) if is_capped else torch.equal(capped[s], free[s])


# ---------------------------------------------------------------------------------------------- 4. configuration, limits, flags, ABI
def test_config_validation():
    d = S.SamplerConfig()
    assert d.score_guidance_sidechains is False and d.score_guidance_max_sc == 0.5
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="score_guidance_max_sc"):
            S.SamplerConfig(score_guidance_max_sc=bad)
    S.SamplerConfig(score_guidance_sidechains=True, score_guidance_max_sc=float("inf"))      # no cap


def _graph(flex=True):
    return make_3dpf_complex(seed=0, flexible_sidechains=flex, n_rec=16)


def _sampler(cfg, flex=True, n=4, sl=None, seed=3):
    g = _graph(flex)
    T, n_sc = int(g["ligand"].edge_mask.sum()), (int(g["flexResidues"].edge_idx.shape[0]) if flex else 0)
    return S.Sampler(Stub(T, n_sc), g, n, torch.device("cpu"), dataclasses.replace(cfg, flexible_sidechains=flex), seed=seed, sample_slice=sl), g


GUIDED = S.SamplerConfig(inference_steps=3, no_random=True, score_guidance_weight=0.5, score_guidance_max_tr=0.4)
BOTH = dataclasses.replace(GUIDED, score_guidance_sidechains=True)


def test_counts_above_the_kernel_limits_raise_at_construction():
    g = _graph()
    n_mov = int(torch.unique(g["flexResidues"].subcomponents).numel())
    n_sc = int(g["flexResidues"].edge_idx.shape[0])
    for name, limit in (("FLEX_MAX_ATOMS", 36), ("FLEX_MAX_TORSIONS", 4), ("FLEX_MAX_MOVING", n_mov - 1), ("FLEX_MAX_BONDS", n_sc - 1)):
        old = getattr(SG, name)
        setattr(SG, name, limit)
        try:
            with pytest.raises(ValueError, match="exceed the limits of ddp_score_guidance_flex"):
                _sampler(BOTH)
            _sampler(GUIDED)                                              # without the flag: not looked at
            _sampler(BOTH, flex=False)                                    # a rigid run: the flag is a no-op
        finally:
            setattr(SG, name, old)
    from diffdock_pocket_amd import _lib as L
    assert (SG.FLEX_MAX_ATOMS, SG.FLEX_MAX_TORSIONS, SG.FLEX_MAX_MOVING, SG.FLEX_MAX_BONDS) == \
        (L.DDP_SCORE_GUIDANCE_FLEX_MAX_ATOMS, L.DDP_SCORE_GUIDANCE_FLEX_MAX_TORSIONS, L.DDP_SCORE_GUIDANCE_FLEX_MAX_MOVING,
         L.DDP_SCORE_GUIDANCE_FLEX_MAX_BONDS) == (512, 1024, 256, 256)


def test_command_line_flags_reach_the_sampler_config():
    from diffdock_pocket_amd.inference import _guidance_fields, _parser
    d = _parser().parse_args([])
    assert d.score_guidance_sidechains is False and d.score_guidance_max_sc == 0.5
    assert S.SamplerConfig(**_guidance_fields(d)) == S.SamplerConfig()
    a = _parser().parse_args(["--score_guidance", "0.75", "--score_guidance_sidechains", "--score_guidance_max_sc", "0.125"])
    cfg = S.SamplerConfig(**_guidance_fields(a))
    assert (cfg.score_guidance_weight, cfg.score_guidance_sidechains, cfg.score_guidance_max_sc) == (0.75, True, 0.125)
    assert cfg.score_guidance_max_tor == 0.5 and cfg.clash_guidance_weight == 0.0


def test_c_abi_declares_the_entry():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import build as B
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "ddp_hip.h")).read()
    assert re.findall(r"^int\s+(ddp_score_guidance_flex)\s*\(", header, flags=re.M) == ["ddp_score_guidance_flex"]
    assert "ddp_score_guidance_flex" in L.EXPORTS and "ddp_score_guidance_flex.hip" in B.SOURCES
    assert os.path.exists(os.path.join(os.path.dirname(B.__file__), "csrc", "ddp_score_guidance_flex.hip"))
    assert set(L.EXPORTS) == set(re.findall(r"^(?:int|const char\*)\s+(ddp_\w+)\s*\(", header, flags=re.M))
    assert "#define DDP_ABI_VERSION 17" in header
    for name, other in (("ATOMS", "DDP_MINIMIZE_MAX_ATOMS"), ("TORSIONS", "DDP_GUIDANCE_MAX_TORSIONS"), ("MOVING", "DDP_MINIMIZE_FLEX_MAX_MOVING"),
                        ("BONDS", "DDP_MINIMIZE_FLEX_MAX_BONDS")):
        assert f"#define DDP_SCORE_GUIDANCE_FLEX_MAX_{name} {other}\n" in header
        assert getattr(L, f"DDP_SCORE_GUIDANCE_FLEX_MAX_{name}") == getattr(L, other)
    # the ctypes struct follows the header's field order
    end = header.index("} ddp_score_guidance_flex_args_t;")
    body = header[header.rindex("typedef struct {", 0, end):end]
    names = re.findall(r"[\s\*]([a-z_]+)(?:\[3\])?[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in L.ScoreGuidanceFlexArgs._fields_]
    assert L.ScoreGuidanceFlexArgs.form.offset == L.ScoreGuidanceArgs.form.offset and L.ScoreGuidanceFlexArgs.form.size == 11 * 8
    assert L.ScoreGuidanceFlexArgs.upd.offset == L.ScoreGuidanceArgs.upd.offset


# ---------------------------------------------------------------------------------------------- 5. the CPU sampler
def sampler_case(smp, pos0, apos0):
    """The restatement's case dict for a sampler's tables and state."""
    tb, sc = smp.sguid_tables, smp.sguid_sc_tables
    return dict(x=pos0.numpy(), y=apos0.numpy(), lig_r=tb.lig_radii.numpy(), lig_f=tb.lig_flags.numpy(), rec_r=tb.rec_radii.numpy(),
                rec_f=tb.rec_flags.numpy(), pairs=tb.self_pairs.numpy(), mov=sc.mov.numpy(), edge=sc.edge_idx.numpy(), sub=sc.sub.numpy(),
                mapping=sc.mapping.numpy(), sc_pairs=sc.pairs.numpy())


def _unguided_sc(cfg, pos0, sched):
    """The side-chain angles the same step applies without the side-chain part, recovered from a sampler that records them."""
    seen = {}
    orig = S.apply_sidechain_torsions

    def spy(pos, edge, sub, mapping, angles):
        seen["sc"] = angles.clone()
        return orig(pos, edge, sub, mapping, angles)

    ref_smp, _ = _sampler(cfg)
    ref_smp.randomize()
    assert torch.equal(ref_smp.lig_pos, pos0)
    S.apply_sidechain_torsions = spy
    try:
        ref_smp.step(0, sched)
    finally:
        S.apply_sidechain_torsions = orig
    return seen["sc"], ref_smp


@pytest.mark.parametrize("ode", [False, True])
def test_one_guided_step_is_the_unguided_update_plus_the_restatement(ode):
    cfg = dataclasses.replace(BOTH, ode=ode)
    sched = get_t_schedule(3)
    smp, g = _sampler(cfg)
    assert smp.score_guidance_sc and smp.sguid_sc_tables.n_sc == smp.S
    smp.randomize()
    pos0, apos0 = smp.lig_pos.clone(), smp.atom_pos.clone()
    base, off = _unguided_sc(dataclasses.replace(cfg, score_guidance_sidechains=False), pos0, sched)
    want = R.forward(sampler_case(smp, pos0, apos0), cfg.score_guidance_weight, cfg.score_guidance_max_sc, base.numpy())
    assert R.margins_ok(want)
    assert float(np.abs(want["inc"]).max()) > 1e-3                      # the term did contribute
    expect = S.apply_sidechain_torsions(apos0, smp.sc_edge_idx, smp.sc_sub, smp.sc_map, torch.from_numpy(want["upd"]))
    smp.step(0, sched)
    d = float((smp.atom_pos - expect).abs().max())
    print(f"[score guidance sc] cpu step ode={ode}: atom_pos differs by {d:.3e} A, capped {want['capped'].tolist()}, moved "
          f"{float((expect - off.atom_pos).abs().max()):.3f} A beyond the step without the side-chain part")
    assert d < 1e-5                                       # the same fp32 side-chain map on increments equal to one rounding
    assert float((expect - off.atom_pos).abs().max()) > 1e-3
    assert torch.equal(smp.lig_pos, off.lig_pos)          # the ligand increments are what they are without the flag, bit for bit


def test_zero_weight_t_above_t_max_and_a_rigid_graph_change_nothing():
    sched = get_t_schedule(3)
    outs = []
    for cfg in (S.SamplerConfig(inference_steps=3, no_random=True),
                S.SamplerConfig(inference_steps=3, no_random=True, score_guidance_sidechains=True, score_guidance_max_sc=0.1),
                S.SamplerConfig(inference_steps=3, no_random=True, score_guidance_weight=2.0, score_guidance_t_max=0.0, score_guidance_sidechains=True)):
        smp, _ = _sampler(cfg)
        assert smp.score_guidance_sc == (cfg.score_guidance_weight > 0) and (smp.score_guidance or not hasattr(smp, "sguid_sc_tables"))
        smp.randomize()
        outs.append(smp.run(sched))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    rigid = []
    for cfg in (GUIDED, BOTH):
        smp, _ = _sampler(cfg, flex=False)
        assert not smp.score_guidance_sc and smp.sguid_sc_tables is None
        smp.randomize()
        rigid.append(smp.run(sched))
    assert torch.equal(rigid[0][0], rigid[1][0]) and torch.equal(rigid[0][1], rigid[1][1])


def test_sliced_samplers_equal_the_whole_sampler_and_clash_guidance_may_be_on():
    sched = get_t_schedule(3)
    cfg = dataclasses.replace(BOTH, clash_guidance_weight=0.5)
    whole, _ = _sampler(cfg)
    whole.randomize()
    lw, aw = whole.run(sched)
    parts = []
    for sl in (slice(0, 2), slice(2, 4)):
        p, _ = _sampler(cfg, sl=sl)
        p.randomize()
        parts.append(p.run(sched))
    assert torch.equal(torch.cat([p[0] for p in parts]), lw) and torch.equal(torch.cat([p[1] for p in parts]), aw)
    off, _ = _sampler(dataclasses.replace(cfg, score_guidance_sidechains=False))
    off.randomize()
    assert not torch.equal(off.run(sched)[1], aw)                        # the side-chain part did move the side chains
