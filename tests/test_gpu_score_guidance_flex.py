"""csrc/ddp_score_guidance_flex.hip on the device: ddp_score_guidance_flex through the C ABI against the float64 restatement of
tests/score_guidance_flex_ref.py, bit for bit against ddp_score_guidance (the ligand part) and ddp_pose_minimize_flex (the side-chain
energy and gradient), with a weight of 0 in device memory, and inside the device sampler.

Bound of the kernel cases, per element of upd_sc (score_guidance_flex_ref.bounds, derived in its docstring): 4 2^-24 (|upd0| +
|increment|) for the three fp32 roundings of the definition plus the fp64 summation bound bgy of flexmin_ref.bounds, carried through
num / den and the cap factor; energy and grad_mov are held to flexmin_ref.bounds alone.  The gradient jumps at the cutoff and at the
ramp ends: every case asserts the margins of score_guidance_flex_ref.margins_ok first (no pair within 1e-6 A of any of them), none is
left out."""
import ctypes as C

import numpy as np
import pytest
import torch

import flexmin_ref as F
import score_guidance_flex_ref as R
from diffdock_pocket_amd.diffusion import get_t_schedule
from test_score_guidance_flex_cpu import CASES, SHAPES, case, case_tables, sampler_case, shape_id

pytestmark = pytest.mark.gpu
CAPS = (1.0, 0.5, 0.5)
TILE_CASE = SHAPES[3]           # (2, 37, 1025, 37, 17): the receptor crosses one LDS tile


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _inputs(c, dev, x=None, y=None):
    x = torch.from_numpy(c["x"]).to(dev) if x is None else x
    y = torch.from_numpy(c["y"]).to(dev).contiguous() if y is None else y
    return x, y


def _launch(c, weight, x=None, y=None, outputs=True, upd0=None, upd0_sc=None):
    """One ddp_score_guidance_flex launch on the case's inputs; returns (upd [3], upd_sc, energy, grad_mov, y) device tensors."""
    from diffdock_pocket_amd.score_guidance import ScoreGuidanceFlexWorkspace
    dev = _dev()
    tb, sc = case_tables(c)
    ws = ScoreGuidanceFlexWorkspace(tb, sc, dev, CAPS, c["max_sc"])
    x, y = _inputs(c, dev, x, y)
    S, T, n_mov, n_sc = x.shape[0], c["bonds"].shape[0], len(c["mov"]), len(c["edge"])
    upd = [torch.from_numpy(np.ascontiguousarray(u)).to(dev) for u in (c["upd0_lig"] if upd0 is None else upd0)]
    upd_sc = torch.from_numpy(np.ascontiguousarray(c["upd0"] if upd0_sc is None else upd0_sc)).to(dev)
    e = torch.full((S, 3), -7.0, dtype=torch.float64, device=dev) if outputs else None
    gm = torch.full((S, n_mov, 3), -7.0, dtype=torch.float64, device=dev) if outputs else None
    w = torch.tensor([weight, 123.0], dtype=torch.float32, device=dev)
    ws.launch(x, y, (upd[0], upd[1], upd[2] if T else None), w[:1], upd_sc if n_sc else None, e, gm)
    torch.cuda.synchronize()
    return upd, upd_sc, e, gm, y


# ---------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("shape", CASES, ids=shape_id)
def test_kernel_matches_the_float64_restatement(shape):
    S, n, m, n_mov, n_sc = shape[:5]
    c = case(shape)
    ref = c["sg"]
    assert R.margins_ok(ref)
    if S > 1 and n_sc and (c["need"] > 0).sum() > 1:
        assert ref["capped"].any() and not ref["capped"].all()          # capped and uncapped samples in one launch
    assert n_sc == 0 or bool((c["upd0"] != 0).all())                    # a non-zero preload
    upd, upd_sc, e, gm, _ = _launch(c, c["w"])
    bu = R.bounds(ref, c["upd0"])
    err = np.abs(upd_sc.cpu().numpy().astype(np.float64) - ref["upd"].astype(np.float64))
    ratio = float((err / np.maximum(bu, 1e-300)).max(initial=0.0))
    be, _, bgy = F.bounds(ref["fm"])
    err_e = np.abs(e.cpu().numpy() - ref["fm"]["energy"][:, :3])
    err_g = np.abs(gm.cpu().numpy() - ref["fm"]["grad_y"])
    re_, rg = float((err_e / be[:, :3]).max()), float((err_g / bgy[:, None, None]).max(initial=0.0))
    print(f"[score guidance sc] {shape} upd_sc: worst err/bound {ratio:.3e} (max |increment| {np.abs(ref['inc']).max(initial=0.0):.3e}), "
          f"energy err/bound {re_:.3e}, grad_mov err/bound {rg:.3e}, capped {ref['capped'].tolist()}")
    assert bool((err <= bu).all()), (shape, ratio)
    assert re_ <= 1.0 and rg <= 1.0, (shape, re_, rg)
    if n_sc == 0:
        assert torch.equal(_bits(upd_sc.cpu()), _bits(torch.from_numpy(c["upd0"])))       # no side chains: untouched
    # a second launch on the same inputs repeats the first bit for bit; without the optional outputs the updates are the same
    upd2, upd_sc2, e2, gm2, _ = _launch(c, c["w"])
    upd3, upd_sc3, _, _, _ = _launch(c, c["w"], outputs=False)
    for a, b, d in zip(upd + [upd_sc], upd2 + [upd_sc2], upd3 + [upd_sc3]):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(d))
    assert torch.equal(_bits(e), _bits(e2)) and torch.equal(_bits(gm), _bits(gm2))


# ---------------------------------------------------------------------------------------------- 2. against ddp_score_guidance
@pytest.mark.parametrize("shape", CASES, ids=shape_id)
def test_ligand_increments_are_the_bits_of_ddp_score_guidance(shape):
    """The same inputs and per-sample receptors: upd_tr, upd_rot, upd_tor and (inter, intra) equal ddp_score_guidance's bit for bit -
    no restraint term touches the ligand gradient here (fx_evaluate's + krest * (x - anchor) would turn a -0.0 into +0.0)."""
    from diffdock_pocket_amd.score_guidance import ScoreGuidanceWorkspace
    dev = _dev()
    c = case(shape)
    S, n, T = shape[0], shape[1], c["bonds"].shape[0]
    upd, _, e, _, y = _launch(c, c["w"])
    tb, _ = case_tables(c)
    ws = ScoreGuidanceWorkspace(tb, dev, CAPS)
    x, _ = _inputs(c, dev)
    want = [torch.from_numpy(u.copy()).to(dev) for u in c["upd0_lig"]]
    e2 = torch.full((S, 2), -7.0, dtype=torch.float64, device=dev)
    ws.launch(x, y, (want[0], want[1], want[2] if T else None), torch.tensor([c["w"]], dtype=torch.float32, device=dev), e2)
    torch.cuda.synchronize()
    for got, w_ in zip(upd, want):
        assert torch.equal(_bits(got), _bits(w_))
    assert torch.equal(_bits(e[:, :2]), _bits(e2))
    if shape[2] >= 1000:                                         # (the crowded cases do interact: the ligand part did act)
        assert not torch.equal(_bits(upd[0].cpu()), _bits(torch.from_numpy(c["upd0_lig"][0])))


# ---------------------------------------------------------------------------------------------- 3. against ddp_pose_minimize_flex
@pytest.mark.parametrize("shape", CASES, ids=shape_id)
def test_side_chain_energy_and_gradient_are_the_bits_of_ddp_pose_minimize_flex(shape):
    """ddp_pose_minimize_flex with iterations = 0, both restraints 0 and anchors equal to the state.  Asserted: BIT equality of sc,
    of grad_mov AND of (inter, intra) with its energy_in - the stronger of the two statements, which contains the bound.  It holds
    because the evaluation is shared without an extra rounding: both kernels call score_evaluate with the same tile patch on the same
    fp32 coordinates and the same fx_second_pass / fx_sc_total of ddp_minimize_flex_loop.h; the minimiser's restraint terms add
    0 * (y - y) = +0.0 to sums that are never -0.0 (every accumulator starts at +0.0)."""
    from diffdock_pocket_amd import launch as LA
    from diffdock_pocket_amd.scoring import ScoreConfig
    dev = _dev()
    c = case(shape)
    S, n, T, n_mov = shape[0], shape[1], c["bonds"].shape[0], len(c["mov"])
    _, _, e, gm, y = _launch(c, c["w"])
    tb, sc = case_tables(c)
    x, _ = _inputs(c, dev)
    tables = LA.flex_tables(sc, c["y"].shape[1], dev)
    step, acc = torch.ones(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)
    e0, e1 = torch.full((S, 6), -7.0, dtype=torch.float64, device=dev), torch.full((S, 6), -7.0, dtype=torch.float64, device=dev)
    gy = torch.full((S, n_mov, 3), -7.0, dtype=torch.float64, device=dev)
    pairs = tb.self_pairs.to(dev) if tb.self_pairs is not None else None
    LA.pose_minimize_flex(x.clone(), x, tb.lig_radii.to(dev), tb.lig_flags.to(dev), y.clone(), y, tb.rec_radii.to(dev), tb.rec_flags.to(dev),
                          ScoreConfig(), pairs, LA.refine_bonds(tb.bonds, n, dev) if T else None,
                          tb.mask_rotate.to(torch.uint8).to(dev) if T else None, tables, step, acc, e0, e1, 0, grad_mov=gy)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e[:, 2]), _bits(e0[:, 2])) and torch.equal(_bits(gm), _bits(gy))
    assert torch.equal(_bits(e[:, :2]), _bits(e0[:, :2]))
    be = F.bounds(c["sg"]["fm"])[0]
    assert bool((np.abs(e.cpu().numpy() - e0[:, :3].cpu().numpy()) <= be[:, :3]).all())          # (contained in the above)


# ---------------------------------------------------------------------------------------------- 4. - 6. zero weight, NaN, read-only
def test_a_zero_weight_in_device_memory_writes_nothing():
    c = case(TILE_CASE)
    upd0 = [u.copy() for u in c["upd0_lig"]]
    upd0[0][1, 1] = float("nan")                                  # (a NaN already in upd keeps its bits as well)
    upd0_sc = c["upd0"].copy()
    upd0_sc[0, 2] = float("nan")
    for w in (0.0, -0.0, float("nan")):
        upd, upd_sc, e, gm, _ = _launch(c, w, upd0=upd0, upd0_sc=upd0_sc)
        for got, u0 in zip(upd + [upd_sc], upd0 + [upd0_sc]):
            assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(u0)))
        assert bool((e == -7.0).all()) and bool((gm == -7.0).all())      # the optional outputs are left alone too


def test_a_nan_in_a_moving_atom_stays_in_its_sample_and_the_receptor_is_only_read():
    shape = SHAPES[2]                                             # (3, 5, 64, 7, 3)
    c = case(shape)
    dev = _dev()
    clean = _launch(c, c["w"])
    y = torch.from_numpy(c["y"]).to(dev).contiguous()
    typed = [int(a) for a in c["mov"] if c["rec_r"][a] >= 0 and c["sc_pairs"][list(c["mov"]).index(a)].any()]
    y[1, typed[0], 0] = float("nan")
    before = y.clone()
    got = _launch(c, c["w"], y=y)
    assert torch.equal(_bits(got[4]), _bits(before))              # the receptor has the same bits after the launch
    assert torch.equal(_bits(clean[4].cpu()), _bits(torch.from_numpy(c["y"])))
    for a, b in zip(clean[0] + list(clean[1:4]), got[0] + list(got[1:4])):
        for s in (0, 2):
            assert torch.equal(_bits(a[s]), _bits(b[s]))
    assert bool(torch.isnan(got[2][1]).any()) and bool(torch.isnan(got[3][1]).any())      # sample 1 is poisoned: energy and gradient


# ---------------------------------------------------------------------------------------------- 7. rejections
def test_abi_rejects_nulls_bad_shapes_and_counts_above_the_limits():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import launch as LA
    from diffdock_pocket_amd.score_guidance import ScoreGuidanceFlexWorkspace
    dev = _dev()
    lib = L.load()
    c = case(TILE_CASE)
    S, n, m, n_mov, n_sc = TILE_CASE
    tb, sc = case_tables(c)
    ws = ScoreGuidanceFlexWorkspace(tb, sc, dev, CAPS, 0.5)
    x, y = _inputs(c, dev)
    upd = [torch.from_numpy(u.copy()).to(dev) for u in c["upd0_lig"]] + [torch.from_numpy(c["upd0"].copy()).to(dev)]
    keep = [u.clone() for u in upd]
    w = torch.tensor([1.0], device=dev)
    ws.launch(x[:0], y[:0], (upd[0][:0], upd[1][:0], upd[2][:0]), w, upd[3][:0])        # n_samples = 0: a no-op
    a = ws.flex_args
    a.n_samples, a.pos, a.weight, a.rec, a.rec_stride = S, x.data_ptr(), w.data_ptr(), y.data_ptr(), 3 * m
    a.upd[0], a.upd[1], a.upd[2], a.upd_sc = (u.data_ptr() for u in upd)

    def call(**over):
        b = L.ScoreGuidanceFlexArgs.from_buffer_copy(a)
        for k, v in over.items():
            if k in ("upd0", "upd1", "upd2"):
                b.upd[int(k[3])] = v
            else:
                setattr(b, k, v)
        return lib.ddp_score_guidance_flex(C.byref(b), LA.stream())

    assert lib.ddp_score_guidance_flex(None, LA.stream()) == -1
    for field in ("pos", "lig_radii", "lig_flags", "rec", "rec_radii", "rec_flags", "bonds", "mask_rotate", "weight", "upd0", "upd1", "upd2",
                  "mov", "sc_pairs", "sc_edge_idx", "sc_map", "sc_sub", "upd_sc"):
        assert call(**{field: None}) == -1, field                # DDP_EINVAL, nothing launched
    assert b"ddp_score_guidance_flex" in lib.ddp_last_error()
    for over in (dict(rec_stride=0), dict(rec_stride=3 * m - 1), dict(n_samples=-1), dict(n=0), dict(m=-1), dict(n_tor=-1), dict(n_mov=-1),
                 dict(n_sc=-1), dict(n_sub=-1), dict(max_tr=-1.0), dict(max_sc=-0.5), dict(max_sc=float("nan")), dict(cutoff=0.0)):
        assert call(**over) == -1, over
    for field, limit in (("n", L.DDP_SCORE_GUIDANCE_FLEX_MAX_ATOMS), ("n_tor", L.DDP_SCORE_GUIDANCE_FLEX_MAX_TORSIONS),
                         ("n_mov", L.DDP_SCORE_GUIDANCE_FLEX_MAX_MOVING), ("n_sc", L.DDP_SCORE_GUIDANCE_FLEX_MAX_BONDS)):
        assert call(**{field: limit + 1}) == -2, field            # DDP_ELIMIT
    assert b"DDP_SCORE_GUIDANCE_FLEX_MAX_BONDS" in lib.ddp_last_error()
    torch.cuda.synchronize()
    for u, k in zip(upd, keep):
        assert torch.equal(_bits(u), _bits(k))                   # none of the refused calls wrote anything
    assert call() == 0
    with pytest.raises(ValueError, match="upd sc"):
        ws.launch(x, y, upd[:3], w, upd[3][:1])
    with pytest.raises(ValueError, match="atom_pos"):
        ws.launch(x, None, upd[:3], w, upd[3])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 8. the device sampler
SEED = 1       # the Sampler seed of tests/test_gpu_score_guidance.py
GUIDED = dict(score_guidance_weight=0.5, score_guidance_max_tr=0.4)
BOTH = dict(score_guidance_sidechains=True, **GUIDED)


def _sampler(graph=False, n=4, sl=None, steps=20, pipelined=False, **fields):
    from diffdock_pocket_amd.sampler import PipelinedSampler, Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    from test_gpu_svgd import _model
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=16)
    cfg = SamplerConfig(inference_steps=steps, flexible_sidechains=True, no_random=True, hip_graph=graph, **fields)
    if pipelined:
        return PipelinedSampler(_model(), g, n, _dev(), cfg, seed=SEED, ways=2), g
    return Sampler(_model(), g, n, _dev(), cfg, seed=SEED, sample_slice=sl), g


def test_one_device_step_matches_the_restatement():
    """One uncaptured guided step: upd_sc = the unguided side-chain update (coefficient x score, no noise) + the restatement's
    increments on the pre-step state, atom_pos = the PyTorch side-chain map of it (2e-4 A, the tolerance of the project's sampler
    tests); the ligand pose equals the flag-off run's bit for bit."""
    from diffdock_pocket_amd import sampler as S
    from diffdock_pocket_amd.score_guidance import ScoreGuidanceFlexWorkspace
    smp, g = _sampler(**BOTH)
    assert isinstance(smp.sguid_ws, ScoreGuidanceFlexWorkspace)
    smp.randomize()
    sched = get_t_schedule(20)
    pos0, apos0 = smp.lig_pos.clone().cpu(), smp.atom_pos.clone().cpu()
    sc_score = smp.scores(float(sched[0]))[3].clone().float().cpu()
    smp.step(0, sched)
    torch.cuda.synchronize()
    _, coef, _ = smp._step_coefficients(0, sched)
    base = (coef[6] * sc_score.reshape(smp.n, smp.S).numpy().astype(np.float64)).astype(np.float32)
    want = R.forward(sampler_case(smp, pos0, apos0), BOTH["score_guidance_weight"], 0.5, base)
    assert R.margins_ok(want)
    assert float(np.abs(want["inc"]).max()) > 1e-3                 # the term did contribute
    dev_k = float(np.abs(smp.upd["sc"].cpu().numpy().astype(np.float64) - want["upd"]).max() / np.abs(want["upd"]).max())
    print(f"[score guidance sc] device step upd_sc: rel_dev {dev_k:.3e}, largest increment {float(np.abs(want['inc']).max()):.3f}, capped "
          f"{want['capped'].tolist()}")
    assert dev_k < 1e-5
    expect = S.apply_sidechain_torsions(apos0, smp.sc_edge_idx, smp.sc_sub.cpu(), smp.sc_map, torch.from_numpy(want["upd"]))
    d = float((smp.atom_pos.cpu() - expect).abs().max())
    print(f"[score guidance sc] device step: atom_pos differs by {d:.3e} A")
    assert d < 2e-4
    off, _ = _sampler(**GUIDED)
    off.randomize()
    off.step(0, sched)
    torch.cuda.synchronize()
    assert torch.equal(smp.lig_pos, off.lig_pos) and not torch.equal(smp.atom_pos, off.atom_pos)


def _run(steps=3, **kw):
    smp, _ = _sampler(**kw)
    smp.randomize()
    sched = get_t_schedule(20)
    for i in range(steps):
        smp.step(i, sched)
    torch.cuda.synchronize()
    used_graph = bool(getattr(smp, "_graph", None))
    out = smp.lig_pos.clone(), smp.atom_pos.clone()
    if hasattr(smp, "close"):
        smp.close()
    return out + (used_graph,)


@pytest.mark.parametrize("fields", [BOTH, dict(clash_guidance_weight=0.5, clash_guidance_max_tr=0.4, **BOTH)], ids=["alone", "with_clash_guidance"])
def test_graph_replay_equals_launch_by_launch_bitwise(fields):
    eager = _run(steps=5, graph=False, **fields)
    replay = _run(steps=5, graph=True, **fields)
    assert not eager[2] and replay[2]
    assert torch.isfinite(eager[0]).all() and torch.equal(eager[0], replay[0]) and torch.equal(eager[1], replay[1])
    assert not torch.equal(replay[1], _run(steps=5, graph=True, **GUIDED)[1])          # the side chains did move


def test_one_captured_graph_replays_across_t_max():
    """get_t_schedule(20) = 1.0, 0.95, 0.9, ...: with t_max = 0.92 the steps 0 and 1 are unguided, the steps from 2 on guided - through
    the one graph that step 0 captured, the weight read from device memory."""
    fields = dict(score_guidance_t_max=0.92, **BOTH)
    sched = get_t_schedule(20)
    assert float(sched[1]) > 0.92 > float(sched[2])
    plain2, two = _run(steps=2, graph=True), _run(steps=2, graph=True, **fields)
    assert torch.equal(plain2[0], two[0]) and torch.equal(plain2[1], two[1])          # not guided yet
    eager, replay = _run(steps=5, graph=False, **fields), _run(steps=5, graph=True, **fields)
    assert replay[2] and torch.equal(eager[0], replay[0]) and torch.equal(eager[1], replay[1])
    assert not torch.equal(replay[1], _run(steps=5, graph=True, score_guidance_t_max=0.92, **GUIDED)[1])      # guided from step 2 on


def test_slices_and_the_pipelined_sampler_equal_the_whole_sampler_bitwise():
    whole = _run(**BOTH)
    parts = [_run(sl=sl, **BOTH) for sl in (slice(0, 2), slice(2, 4))]
    pipe = _run(pipelined=True, **BOTH)
    cat = [torch.cat([p[k] for p in parts]) for k in (0, 1)]
    assert torch.equal(pipe[0], cat[0]) and torch.equal(pipe[1], cat[1])
    assert torch.equal(cat[0], whole[0]) and torch.equal(cat[1], whole[1])
