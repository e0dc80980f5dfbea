"""csrc/ddp_score_guidance.hip on the device: ddp_score_guidance through the C ABI against the float64 restatement of
tests/score_guidance_ref.py, bit for bit against ddp_pose_score + ddp_refine_direction, with a weight of 0 in device memory, and inside
the device sampler.

Bound of the kernel cases, per element of upd (score_guidance_ref.bounds): 4 2^-24 (|upd0| + |increment|) for the fp32 roundings of
the definition (direction, increment, sum) plus the fp64 summation bound 256 eps (P + 1) max(1, largest pair term) of
vinardo_ref.bounds, carried through the ratios of the direction and the cap factor by guidance_ref.bounds; the energy and gradient
outputs are held to the fp64 bound alone.  The gradient of the score jumps at the cutoff and at the ramp ends: every case asserts the
margins of score_guidance_ref.margins_ok first (no pair within 1e-6 A of any of them), none is left out."""
import ctypes as C

import numpy as np
import pytest
import torch

import score_guidance_ref as R
from diffdock_pocket_amd.diffusion import get_t_schedule
from diffdock_pocket_amd.scoring import ScoreConfig
from test_score_guidance_cpu import LIMIT_SHAPE, SHAPES, case, case_tables, shape_id

pytestmark = pytest.mark.gpu
INF = float("inf")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _launch(c, weight, caps, upd0, x=None, outputs=True):
    """One ddp_score_guidance launch on the case's inputs; returns (upd [3], energy, grad) device tensors."""
    from diffdock_pocket_amd.score_guidance import ScoreGuidanceWorkspace
    dev = _dev()
    ws = ScoreGuidanceWorkspace(case_tables(c), dev, caps)
    x = torch.from_numpy(c["x"]).to(dev) if x is None else x
    S, n, T = x.shape[0], x.shape[1], c["bonds"].shape[0]
    rec = torch.from_numpy(c["rec"]).to(dev).contiguous() if c["rec"].ndim == 3 else None
    upd = [torch.from_numpy(np.ascontiguousarray(u)).to(dev) for u in upd0]
    e = torch.full((S, 2), -7.0, dtype=torch.float64, device=dev) if outputs else None
    g = torch.full((S, n, 3), -7.0, dtype=torch.float64, device=dev) if outputs else None
    w = torch.tensor([weight, 123.0], dtype=torch.float32, device=dev)
    ws.launch(x, rec, (upd[0], upd[1], upd[2] if T else None), w[:1], e, g)
    torch.cuda.synchronize()
    return upd, e, g


# ---------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("shape", SHAPES + [LIMIT_SHAPE], ids=shape_id)
def test_kernel_matches_the_float64_restatement(shape):
    S, n, m, T, per_sample, with_pairs = shape
    c = case(shape)
    ref = c["ref"]
    assert R.margins_ok(ref, n)
    if S > 1 and (c["need"] > 0).sum() > 1:
        assert ref["capped"].any() and not ref["capped"].all()          # capped and uncapped samples in one launch
    upd, e, g = _launch(c, c["w"], c["caps"], c["upd0"])
    be, bg, bu = R.bounds(ref, n, c["upd0"])
    worst = 0.0
    for k, name in enumerate(("tr", "rot", "tor")):
        err = np.abs(upd[k].cpu().numpy().astype(np.float64) - ref["upd"][k].astype(np.float64))
        ratio = float((err / np.maximum(bu[k], 1e-300)).max(initial=0.0))
        worst = max(worst, ratio)
        print(f"[score guidance] {shape} upd_{name}: worst err/bound {ratio:.3e} (max |increment| {np.abs(ref['inc'][k]).max(initial=0.0):.3e})")
        assert bool((err <= bu[k]).all()), (shape, name, ratio)
    err_e = np.abs(e.cpu().numpy() - ref["eg"]["e"])
    err_g = np.abs(g.cpu().numpy() - ref["eg"]["g"])
    re_, rg = float((err_e / be).max()), float((err_g / bg[:, None, None]).max())
    print(f"[score guidance] {shape} energy err/bound {re_:.3e}, gradient err/bound {rg:.3e}, upd worst {worst:.3e}, capped {ref['capped'].tolist()}")
    assert re_ <= 1.0 and rg <= 1.0, (shape, re_, rg)
    if m == 0:
        assert bool((e[:, 0] == 0).all())
    # a second launch on the same inputs repeats the first bit for bit; without the optional outputs the updates are the same
    upd2, e2, g2 = _launch(c, c["w"], c["caps"], c["upd0"])
    upd3, _, _ = _launch(c, c["w"], c["caps"], c["upd0"], outputs=False)
    for a, b, d in zip(upd, upd2, upd3):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(d))
    assert torch.equal(_bits(e), _bits(e2)) and torch.equal(_bits(g), _bits(g2))


def test_one_launch_holds_capped_and_uncapped_samples():
    shape = (4, 37, 1025, 7, True, True)
    ref = case(shape)["ref"]
    assert ref["capped"].any() and not ref["capped"].all()


# ---------------------------------------------------------------------------------------------- 2. against the existing kernels
@pytest.mark.parametrize("n", [1, 5, 37, 256])
@pytest.mark.parametrize("m", [0, 1, 1025])
def test_bits_equal_pose_score_then_refine_direction(n, m):
    """Caps of +infinity and upd = 0: the increments are ddp_refine_direction's for step[s] = w on the gradient of ddp_pose_score, bit
    for bit (pushed through the same fp32 sum 0 + d), and so are the gradient and the energies (inter, intra)."""
    from diffdock_pocket_amd import launch as LA
    dev = _dev()
    S, T = 3, (0 if n == 1 else 5)
    c = R.random_case(S, n, m, T, seed=77 + 1000 * n + m, per_sample_rec=(m == 1025), with_pairs=True)
    assert R.margins_ok(c["ref"], n)
    tb = case_tables(c)
    zero = [np.zeros((S, 3), np.float32), np.zeros((S, 3), np.float32), np.zeros((S, T), np.float32)]
    upd, e, g = _launch(c, c["w"], (INF, INF, INF), zero)
    x = torch.from_numpy(c["x"]).to(dev)
    rec = tb.rec.to(dev).contiguous()
    e7, gr = LA.pose_score(x, tb.lig_radii.to(dev), tb.lig_flags.to(dev), rec, tb.rec_radii.to(dev), tb.rec_flags.to(dev), tb.config, 1.0,
                           tb.self_pairs.to(dev), with_grad=True)
    tr, rot, tor = torch.full((S, 3), -7.0, device=dev), torch.full((S, 3), -7.0, device=dev), torch.full((S, T), -7.0, device=dev)
    step = torch.full((S,), float(np.float32(c["w"])), dtype=torch.float64, device=dev)
    a = LA.refine_args(x, x, tb.lig_radii.to(dev), rec, tb.rec_radii.to(dev), tb.self_pairs.to(dev), 0.4, 0.0, None, gr,
                       bonds=LA.refine_bonds(tb.bonds, n, dev) if T else None,
                       mask_rotate=tb.mask_rotate.to(torch.uint8).to(dev) if T else None, step=step, tr=tr, rot=rot, tor=tor if T else None)
    LA.refine_direction(a)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g), _bits(gr)) and torch.equal(_bits(e), _bits(e7[:, 4:6]))
    for got, d in zip(upd[:3 if T else 2], (tr, rot, tor)):
        assert torch.equal(_bits(got), _bits(torch.zeros_like(d) + d))
    assert bool(torch.isfinite(tr).all()) and (m < 1025 or float(tr.abs().max()) > 0)      # (the crowded cases do interact)


# ---------------------------------------------------------------------------------------------- 3. zero weight and NaN
def test_a_zero_weight_in_device_memory_writes_nothing_and_nan_stays_in_its_sample():
    shape = (4, 37, 1025, 7, True, True)
    c = case(shape)
    dev = _dev()
    x = torch.from_numpy(c["x"]).to(dev)
    bad = x.clone()
    bad[1, int(np.nonzero(c["lig_r"] >= 0)[0][0]), 0] = float("nan")      # a typed atom: the NaN rule of the score
    upd0 = [u.copy() for u in c["upd0"]]
    upd0[0][2, 1] = float("nan")                                  # (a NaN already in upd keeps its bits as well)
    for w in (0.0, -0.0):
        upd, e, g = _launch(c, w, c["caps"], upd0, x=bad)
        for got, u0 in zip(upd, upd0):
            assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(u0)))
        assert bool((e == -7.0).all()) and bool((g == -7.0).all())      # the optional outputs are left alone too
    clean, e0, g0 = _launch(c, c["w"], c["caps"], c["upd0"])
    got, e1, g1 = _launch(c, c["w"], c["caps"], c["upd0"], x=bad)
    for k, (a, b) in enumerate(zip(got, clean)):
        # (the translation and the rotation sum over every atom - the centroid is NaN; a torsion is NaN where its axis or levers are)
        assert bool(torch.isnan(a[1]).all()) if k < 2 else bool(torch.isnan(a[1]).any())
        for s in (0, 2, 3):
            assert torch.equal(_bits(a[s]), _bits(b[s]))
    keep = [0, 2, 3]
    assert torch.equal(_bits(e1[keep]), _bits(e0[keep])) and torch.equal(_bits(g1[keep]), _bits(g0[keep]))
    assert bool(torch.isnan(e1[1]).any())


# ---------------------------------------------------------------------------------------------- 4. rejections
def test_abi_rejects_nulls_bad_shapes_bad_constants_and_ligands_above_the_limit():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import launch as LA
    from diffdock_pocket_amd.score_guidance import ScoreGuidanceWorkspace
    dev = _dev()
    lib = L.load()
    shape = (4, 37, 1025, 7, True, True)
    c = case(shape)
    ws = ScoreGuidanceWorkspace(case_tables(c), dev)
    x = torch.from_numpy(c["x"]).to(dev)
    rec = torch.from_numpy(c["rec"]).to(dev).contiguous()
    upd = [torch.from_numpy(u.copy()).to(dev) for u in c["upd0"]]
    keep = [u.clone() for u in upd]
    w = torch.tensor([1.0], device=dev)
    ws.launch(x[:0], rec[:0], (upd[0][:0], upd[1][:0], upd[2][:0]), w)        # n_samples = 0: a no-op
    a = ws.args
    a.n_samples, a.pos, a.weight = 4, x.data_ptr(), w.data_ptr()
    a.upd[0], a.upd[1], a.upd[2] = (u.data_ptr() for u in upd)
    a.rec, a.rec_stride = rec.data_ptr(), 3 * 1025

    def call(**over):
        b = L.ScoreGuidanceArgs.from_buffer_copy(a)
        for k, v in over.items():
            if k.startswith("upd"):
                b.upd[int(k[3])] = v
            else:
                setattr(b, k, v)
        return lib.ddp_score_guidance(C.byref(b), LA.stream())

    assert lib.ddp_score_guidance(None, LA.stream()) == -1
    for field in ("pos", "lig_radii", "lig_flags", "rec", "rec_radii", "rec_flags", "bonds", "mask_rotate", "weight", "upd0", "upd1", "upd2"):
        assert call(**{field: None}) == -1, field                # DDP_EINVAL, nothing launched
    for over in (dict(n_samples=-1), dict(n=0), dict(m=-1), dict(n_tor=-1), dict(rec_stride=3 * 1025 - 1), dict(max_tr=-1.0),
                 dict(max_rot=float("nan")), dict(max_tor=-0.5), dict(cutoff=0.0), dict(cutoff=INF), dict(gauss_width=0.0),
                 dict(hydrophobic_bad=-1.0), dict(hbond_good=1.0)):
        assert call(**over) == -1, over
    assert b"ddp_score_guidance" in lib.ddp_last_error()
    assert call(n=L.DDP_EVAL_MAX_ATOMS + 1) == -2                # DDP_ELIMIT
    assert call(n_tor=L.DDP_GUIDANCE_MAX_TORSIONS + 1) == -2
    assert b"DDP_GUIDANCE_MAX_TORSIONS" in lib.ddp_last_error()
    torch.cuda.synchronize()
    for u, k in zip(upd, keep):
        assert torch.equal(_bits(u), _bits(k))                   # none of the refused calls wrote anything
    assert call() == 0
    with pytest.raises(ValueError, match="upd rot"):
        ws.launch(x, rec, (upd[0], upd[1][:2], upd[2]), w)
    with pytest.raises(ValueError, match="weight"):
        ws.launch(x, rec, upd, w.cpu())
    torch.cuda.synchronize()


def test_sampler_raises_for_a_ligand_above_the_limit():
    from diffdock_pocket_amd import score_guidance as SG
    from diffdock_pocket_amd.sampler import Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    g = make_3dpf_complex(seed=0, flexible_sidechains=False)
    old = SG.MAX_ATOMS
    SG.MAX_ATOMS = 36            # the 3dpf ligand has 37 atoms (a ligand of 1025 atoms has no place in a quick test)
    try:
        with pytest.raises(ValueError, match="exceeds the limits"):
            Sampler(None, g, 2, _dev(), SamplerConfig(flexible_sidechains=False, score_guidance_weight=1.0))
    finally:
        SG.MAX_ATOMS = old


# ---------------------------------------------------------------------------------------------- the device sampler
SEED = 1       # the Sampler seed of tests/test_gpu_guidance.py; its start poses keep the margins of the score as well (checked below)
GUIDED = dict(score_guidance_weight=0.5, score_guidance_max_tr=0.4)


def _sampler(flex=False, graph=False, n=4, sl=None, steps=20, pipelined=False, **fields):
    from diffdock_pocket_amd.sampler import PipelinedSampler, Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    from test_gpu_svgd import _model
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=16)
    cfg = SamplerConfig(inference_steps=steps, flexible_sidechains=flex, no_random=True, hip_graph=graph, **fields)
    if pipelined:
        return PipelinedSampler(_model(), g, n, _dev(), cfg, seed=SEED, ways=2), g
    return Sampler(_model(), g, n, _dev(), cfg, seed=SEED, sample_slice=sl), g


# ---------------------------------------------------------------------------------------------- 5. one device step
@pytest.mark.parametrize("flex", [False, True])
def test_one_device_step_matches_the_restatement(flex):
    """One uncaptured guided step = the unguided updates (coefficients x scores(t), no noise) + the restatement's increments on the
    pre-step poses, then the PyTorch modify_conformer: 2e-4 A, the tolerance of the project's sampler tests."""
    from diffdock_pocket_amd import sampler as S
    smp, g = _sampler(flex=flex, **GUIDED)
    smp.randomize()
    sched = get_t_schedule(20)
    pos0, apos0 = smp.lig_pos.clone().cpu(), smp.atom_pos.clone().cpu()
    sc = [s.clone().float().cpu() for s in smp.scores(float(sched[0]))]
    smp.step(0, sched)
    torch.cuda.synchronize()
    T, tb = smp.T, smp.sguid_tables
    _, coef, _ = smp._step_coefficients(0, sched)
    base = [(coef[0] * sc[0].numpy().astype(np.float64)).astype(np.float32), (coef[2] * sc[1].numpy().astype(np.float64)).astype(np.float32),
            (coef[4] * sc[2].reshape(smp.n, T).numpy().astype(np.float64)).astype(np.float32)]
    want = R.forward(pos0.numpy(), tb.lig_radii.numpy(), tb.lig_flags.numpy(), apos0.numpy() if flex else tb.rec.numpy(), tb.rec_radii.numpy(),
                     tb.rec_flags.numpy(), tb.self_pairs.numpy(), tb.bonds.numpy(), tb.mask_rotate.numpy(), GUIDED["score_guidance_weight"],
                     (0.4, 0.5, 0.5), base)
    assert R.margins_ok(want, smp.n_l)
    big = max(float(np.abs(i).max()) for i in want["inc"])
    assert big > 1e-3                                            # the term did contribute
    for k, name in enumerate(("tr", "rot", "tor")):
        dev_k = R.rel_dev(smp.upd[name].cpu().numpy(), want["upd"][k])
        print(f"[score guidance] device step flex={flex} upd_{name}: rel_dev {dev_k:.3e}")
        assert dev_k < 1e-5, name                                # (the step did use these updates)
    upd = [torch.from_numpy(u) for u in want["upd"]]
    expect = S.modify_conformer(pos0, upd[0], upd[1], upd[2], smp.bonds, [i.cpu() for i in smp.rot_idx])
    d = float((smp.lig_pos.cpu() - expect).abs().max())
    print(f"[score guidance] device step flex={flex}: poses differ by {d:.3e} A; largest increment {big:.3f}, capped {want['capped'].tolist()}")
    assert d < 2e-4


# ---------------------------------------------------------------------------------------------- 6. graph replay
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


BOTH = dict(clash_guidance_weight=0.5, clash_guidance_max_tr=0.4, **GUIDED)


@pytest.mark.parametrize("flex,fields", [(False, GUIDED), (True, GUIDED), (False, BOTH)], ids=["rigid", "flex", "rigid_with_clash_guidance"])
def test_graph_replay_equals_launch_by_launch_bitwise(flex, fields):
    eager = _run(steps=5, flex=flex, graph=False, **fields)
    replay = _run(steps=5, flex=flex, graph=True, **fields)
    assert not eager[2] and replay[2]
    assert torch.isfinite(eager[0]).all() and torch.equal(eager[0], replay[0]) and torch.equal(eager[1], replay[1])
    if fields is BOTH:                                           # both terms act: neither alone gives these poses
        assert not torch.equal(replay[0], _run(steps=5, flex=flex, graph=True, **GUIDED)[0])


def test_one_captured_graph_replays_across_t_max():
    """get_t_schedule(20) = 1.0, 0.95, 0.9, ...: with t_max = 0.92 the steps 0 and 1 are unguided, the steps from 2 on guided - through
    the one graph that step 0 captured, the weight read from device memory."""
    fields = dict(score_guidance_t_max=0.92, **GUIDED)
    sched = get_t_schedule(20)
    assert float(sched[1]) > 0.92 > float(sched[2])
    plain2, two = _run(steps=2, graph=True), _run(steps=2, graph=True, **fields)
    assert torch.equal(plain2[0], two[0]) and torch.equal(plain2[1], two[1])          # not guided yet
    eager, replay = _run(steps=5, graph=False, **fields), _run(steps=5, graph=True, **fields)
    assert replay[2] and torch.equal(eager[0], replay[0]) and torch.equal(eager[1], replay[1])
    assert not torch.equal(replay[0], _run(steps=5, graph=True)[0])                   # guided from step 2 on


# ---------------------------------------------------------------------------------------------- 7. slices and the pipelined sampler
@pytest.mark.parametrize("flex", [False, True])
def test_slices_and_the_pipelined_sampler_equal_the_whole_sampler_bitwise(flex):
    whole = _run(flex=flex, **GUIDED)
    parts = [_run(flex=flex, sl=sl, **GUIDED) for sl in (slice(0, 2), slice(2, 4))]
    pipe = _run(flex=flex, pipelined=True, **GUIDED)
    cat = [torch.cat([p[k] for p in parts]) for k in (0, 1)]
    print(f"[score guidance] flex={flex}: slices vs whole {float((cat[0] - whole[0]).abs().max()):.3e} A, pipelined vs whole "
          f"{float((pipe[0] - whole[0]).abs().max()):.3e} A, pipelined vs slices {float((pipe[0] - cat[0]).abs().max()):.3e} A")
    assert torch.equal(pipe[0], cat[0]) and torch.equal(pipe[1], cat[1])
    assert torch.equal(cat[0], whole[0]) and torch.equal(cat[1], whole[1])
    assert torch.equal(pipe[0], whole[0]) and torch.equal(pipe[1], whole[1])


def test_t_max_below_every_t_equals_the_unguided_sampler_through_the_graph():
    plain = _run(steps=5, graph=True)
    off = _run(steps=5, graph=True, score_guidance_weight=2.0, score_guidance_t_max=0.0)
    guided = _run(steps=5, graph=True, **GUIDED)
    assert torch.equal(plain[0], off[0]) and torch.equal(plain[1], off[1])
    assert not torch.equal(plain[0], guided[0])
