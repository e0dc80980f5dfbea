"""csrc/ddp_guidance.hip on the device: ddp_clash_guidance through the C ABI against the float64 restatement of tests/guidance_ref.py,
bit for bit against ddp_refine_energy + ddp_refine_direction, with a weight of 0 in device memory, and inside the device sampler.

Bound of the kernel cases, per element of upd (guidance_ref.bounds): 4 2^-24 (|upd0| + |increment|) for the fp32 roundings of the
definition (direction, increment, sum) plus the fp64 summation bound 256 eps (P + 1) x largest term of the pair sums, carried through
the ratios of the direction and the cap factor; the energy and gradient outputs are held to the fp64 bound alone.  No case is left
out for a discontinuity (the energy is C1, min() is continuous): every case asserts the margins of guidance_ref.margins_ok first."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import guidance_ref as R
from diffdock_pocket_amd.diffusion import get_t_schedule
from test_guidance_cpu import SHAPES, case_tables

pytestmark = pytest.mark.gpu
INF = float("inf")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


@functools.lru_cache(maxsize=None)
def _case(shape):
    S, n, m, T, per_sample, with_pairs = shape
    return R.random_case(S, n, m, T, seed=1000 * n + m + T + S, per_sample_rec=per_sample, with_pairs=with_pairs)


def _launch(c, weight, caps, upd0, x=None, outputs=True):
    """One ddp_clash_guidance launch on the case's inputs; returns (upd [3], energy, grad) device tensors."""
    from diffdock_pocket_amd.guidance import GuidanceWorkspace
    dev = _dev()
    ws = GuidanceWorkspace(case_tables(c), dev, *caps)
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


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "S{}_n{}_m{}_T{}_{}_{}".format(*s))
def test_kernel_matches_the_float64_restatement(shape):
    S, n, m, T, per_sample, with_pairs = shape
    c = _case(shape)
    ref = c["ref"]
    assert R.margins_ok(ref, n)
    if S > 1 and (c["need"] > 0).sum() > 1 and c["need"].max() > c["need"][c["need"] > 0].min():
        assert ref["capped"].any() and not ref["capped"].all()          # capped and uncapped samples in one launch
    upd, e, g = _launch(c, c["w"], c["caps"], c["upd0"])
    be, bg, bu = R.bounds(ref, n, c["upd0"])
    worst = 0.0
    for k, name in enumerate(("tr", "rot", "tor")):
        err = np.abs(upd[k].cpu().numpy().astype(np.float64) - ref["upd"][k].astype(np.float64))
        ratio = float((err / np.maximum(bu[k], 1e-300)).max(initial=0.0))
        worst = max(worst, ratio)
        print(f"[guidance] {shape} upd_{name}: worst err/bound {ratio:.3e} (max |increment| {np.abs(ref['inc'][k]).max(initial=0.0):.3e})")
        assert bool((err <= bu[k]).all()), (shape, name, ratio)
    err_e = np.abs(e.cpu().numpy() - ref["eg"]["e"])
    err_g = np.abs(g.cpu().numpy() - ref["eg"]["g"])
    re_, rg = float((err_e / be[:, None]).max()), float((err_g / bg[:, None, None]).max())
    print(f"[guidance] {shape} energy err/bound {re_:.3e}, gradient err/bound {rg:.3e}, upd worst {worst:.3e}, capped {ref['capped'].tolist()}")
    assert re_ <= 1.0 and rg <= 1.0, (shape, re_, rg)
    if m == 0:
        assert bool((e[:, 0] == 0).all())
    # a second launch on the same inputs repeats the first bit for bit; without the optional outputs the updates are the same
    upd2, e2, g2 = _launch(c, c["w"], c["caps"], c["upd0"])
    upd3, _, _ = _launch(c, c["w"], c["caps"], c["upd0"], outputs=False)
    for a, b, d in zip(upd, upd2, upd3):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(d))
    assert torch.equal(_bits(e), _bits(e2)) and torch.equal(_bits(g), _bits(g2))


@pytest.mark.parametrize("n", [1, 5, 37, 256])
@pytest.mark.parametrize("m", [0, 1, 1025])
def test_bits_equal_refine_energy_then_refine_direction(n, m):
    """Caps of +infinity and upd = 0: the increments are ddp_refine_direction's for step[s] = w on the gradient of ddp_refine_energy
    (restraint 0, anchor = pose), bit for bit (pushed through the same fp32 sum 0 + d), and so are the gradient and the energies."""
    from diffdock_pocket_amd import launch as LA
    dev = _dev()
    S, T = 3, (0 if n == 1 else 5)
    c = R.random_case(S, n, m, T, seed=77 + 1000 * n + m, per_sample_rec=(m == 1025), with_pairs=True)
    tb = case_tables(c)
    zero = [np.zeros((S, 3), np.float32), np.zeros((S, 3), np.float32), np.zeros((S, T), np.float32)]
    upd, e, g = _launch(c, c["w"], (INF, INF, INF), zero)
    x = torch.from_numpy(c["x"]).to(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    e4, gr = torch.empty(S, 4, **f64), torch.empty(S, n, 3, **f64)
    tr, rot, tor = torch.full((S, 3), -7.0, device=dev), torch.full((S, 3), -7.0, device=dev), torch.full((S, T), -7.0, device=dev)
    step = torch.full((S,), float(np.float32(c["w"])), **f64)
    a = LA.refine_args(x, x, tb.lig_radii.to(dev), tb.rec.to(dev).contiguous(), tb.rec_radii.to(dev), tb.self_pairs.to(dev), R.OVERLAP, 0.0,
                       e4, gr, bonds=LA.refine_bonds(tb.bonds, n, dev) if T else None,
                       mask_rotate=tb.mask_rotate.to(torch.uint8).to(dev) if T else None, step=step, tr=tr, rot=rot, tor=tor if T else None)
    LA.refine_energy(a)
    LA.refine_direction(a)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g), _bits(gr)) and torch.equal(_bits(e), _bits(e4[:, :2]))
    for got, d in zip(upd[:3 if T else 2], (tr, rot, tor)):
        assert torch.equal(_bits(got), _bits(torch.zeros_like(d) + d))
    assert bool(torch.isfinite(tr).all()) and (m < 1025 or float(tr.abs().max()) > 0)      # (the crowded cases do clash)


def test_a_zero_weight_in_device_memory_writes_nothing_and_nan_stays_in_its_sample():
    shape = (3, 37, 1025, 5, False, True)
    c = _case(shape)
    dev = _dev()
    x = torch.from_numpy(c["x"]).to(dev)
    bad = x.clone()
    bad[1, 3, 0] = float("nan")
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
        # (the translation and the rotation sum over every atom; a torsion whose atoms and pairs avoid the NaN atom stays finite)
        assert bool(torch.isnan(a[1]).all()) if k < 2 else bool(torch.isnan(a[1]).any())
        for s in (0, 2):
            assert torch.equal(_bits(a[s]), _bits(b[s]))
    assert bool(torch.isnan(e1[1, 0])) and torch.equal(_bits(e1[[0, 2]]), _bits(e0[[0, 2]])) and torch.equal(_bits(g1[[0, 2]]), _bits(g0[[0, 2]]))


def test_abi_rejects_nulls_bad_shapes_and_ligands_above_the_limit():
    from diffdock_pocket_amd import _lib as L
    from diffdock_pocket_amd import launch as LA
    from diffdock_pocket_amd.guidance import GuidanceWorkspace
    dev = _dev()
    lib = L.load()
    c = _case((3, 37, 1025, 5, False, True))
    ws = GuidanceWorkspace(case_tables(c), dev)
    x = torch.from_numpy(c["x"]).to(dev)
    upd = [torch.from_numpy(u.copy()).to(dev) for u in c["upd0"]]
    keep = [u.clone() for u in upd]
    w = torch.tensor([1.0], device=dev)
    ws.launch(x[:0], None, (upd[0][:0], upd[1][:0], upd[2][:0]), w)        # n_samples = 0: a no-op
    a = ws.args
    a.n_samples, a.pos, a.weight = 3, x.data_ptr(), w.data_ptr()
    a.upd[0], a.upd[1], a.upd[2] = (u.data_ptr() for u in upd)
    a.rec, a.rec_stride = ws.rec.data_ptr(), 0

    def call(**over):
        b = L.GuidanceArgs.from_buffer_copy(a)
        for k, v in over.items():
            if k.startswith("upd"):
                b.upd[int(k[3])] = v
            else:
                setattr(b, k, v)
        return lib.ddp_clash_guidance(C.byref(b), LA.stream())

    assert lib.ddp_clash_guidance(None, LA.stream()) == -1
    for field in ("pos", "lig_radii", "rec", "rec_radii", "bonds", "mask_rotate", "weight", "upd0", "upd1", "upd2"):
        assert call(**{field: None}) == -1, field                # DDP_EINVAL, nothing launched
    for over in (dict(n_samples=-1), dict(n=0), dict(m=-1), dict(n_tor=-1), dict(rec_stride=3 * 1025 - 1), dict(max_tr=-1.0),
                 dict(max_rot=float("nan")), dict(max_tor=-0.5), dict(overlap=INF)):
        assert call(**over) == -1, over
    assert call(n=L.DDP_EVAL_MAX_ATOMS + 1) == -2                # DDP_ELIMIT
    assert call(n_tor=L.DDP_GUIDANCE_MAX_TORSIONS + 1) == -2
    assert b"DDP_GUIDANCE_MAX_TORSIONS" in lib.ddp_last_error()
    torch.cuda.synchronize()
    for u, k in zip(upd, keep):
        assert torch.equal(_bits(u), _bits(k))                   # none of the refused calls wrote anything
    assert call() == 0
    with pytest.raises(ValueError, match="upd rot"):
        ws.launch(x, None, (upd[0], upd[1][:2], upd[2]), w)
    with pytest.raises(ValueError, match="weight"):
        ws.launch(x, None, upd, w.cpu())
    torch.cuda.synchronize()


def test_sampler_raises_for_a_ligand_above_the_limit():
    from diffdock_pocket_amd import guidance as G
    from diffdock_pocket_amd.sampler import Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    g = make_3dpf_complex(seed=0, flexible_sidechains=False)
    old = G.MAX_ATOMS
    G.MAX_ATOMS = 36            # the 3dpf ligand has 37 atoms (a ligand of 1025 atoms has no place in a quick test)
    try:
        with pytest.raises(ValueError, match="exceeds the limits"):
            Sampler(None, g, 2, _dev(), SamplerConfig(flexible_sidechains=False, clash_guidance_weight=1.0))
    finally:
        G.MAX_ATOMS = old


# ---------------------------------------------------------------------------------------------- the device sampler
SEED = 1       # Sampler seed whose start poses (no_random: torsions and rotations only) clash with the pocket and keep the margins; found on the CPU
GUIDED = dict(clash_guidance_weight=0.5, clash_guidance_max_tr=0.4)


def _sampler(flex=False, graph=False, n=4, sl=None, steps=20, pipelined=False, **fields):
    from diffdock_pocket_amd.sampler import PipelinedSampler, Sampler, SamplerConfig
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    from test_gpu_svgd import _model
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_rec=16)
    cfg = SamplerConfig(inference_steps=steps, flexible_sidechains=flex, no_random=True, hip_graph=graph, **fields)
    if pipelined:
        return PipelinedSampler(_model(), g, n, _dev(), cfg, seed=SEED, ways=2), g
    return Sampler(_model(), g, n, _dev(), cfg, seed=SEED, sample_slice=sl), g


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
    T, tb = smp.T, smp.guid_tables
    _, coef, _ = smp._step_coefficients(0, sched)
    base = [(coef[0] * sc[0].numpy().astype(np.float64)).astype(np.float32), (coef[2] * sc[1].numpy().astype(np.float64)).astype(np.float32),
            (coef[4] * sc[2].reshape(smp.n, T).numpy().astype(np.float64)).astype(np.float32)]
    want = R.forward(pos0.numpy(), tb.lig_radii.numpy(), apos0.numpy() if flex else tb.rec.numpy(), tb.rec_radii.numpy(),
                     tb.self_pairs.numpy(), tb.bonds.numpy(), tb.mask_rotate.numpy(), GUIDED["clash_guidance_weight"], (0.4, 0.5, 0.5), base)
    assert R.margins_ok(want, smp.n_l)
    big = max(float(np.abs(i).max()) for i in want["inc"])
    assert big > 1e-3                                            # the term did contribute
    for k, name in enumerate(("tr", "rot", "tor")):
        dev_k = R.rel_dev(smp.upd[name].cpu().numpy(), want["upd"][k])
        print(f"[guidance] device step flex={flex} upd_{name}: rel_dev {dev_k:.3e}")
        assert dev_k < 1e-5, name                                # (the step did use these updates)
    upd = [torch.from_numpy(u) for u in want["upd"]]
    expect = S.modify_conformer(pos0, upd[0], upd[1], upd[2], smp.bonds, [i.cpu() for i in smp.rot_idx])
    d = float((smp.lig_pos.cpu() - expect).abs().max())
    print(f"[guidance] device step flex={flex}: poses differ by {d:.3e} A; largest increment {big:.3f}, capped {want['capped'].tolist()}")
    assert d < 2e-4


@pytest.mark.parametrize("flex", [False, True])
def test_graph_replay_equals_launch_by_launch_bitwise(flex):
    sched = get_t_schedule(20)
    out = []
    for graph in (False, True):
        smp, _ = _sampler(flex=flex, graph=graph, **GUIDED)
        smp.randomize()
        for i in range(5):
            smp.step(i, sched)
        torch.cuda.synchronize()
        assert bool(smp._graph) == graph
        out.append((smp.lig_pos.clone(), smp.atom_pos.clone()))
        smp.close()
    assert torch.isfinite(out[0][0]).all() and torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def _run(steps=3, **kw):
    smp, _ = _sampler(**kw)
    smp.randomize()
    sched = get_t_schedule(20)
    for i in range(steps):
        smp.step(i, sched)
    torch.cuda.synchronize()
    out = smp.lig_pos.clone(), smp.atom_pos.clone()
    if hasattr(smp, "close"):
        smp.close()
    return out


@pytest.mark.parametrize("flex", [False, True])
def test_slices_and_the_pipelined_sampler_equal_the_whole_sampler_bitwise(flex):
    whole = _run(flex=flex, **GUIDED)
    parts = [_run(flex=flex, sl=sl, **GUIDED) for sl in (slice(0, 2), slice(2, 4))]
    pipe = _run(flex=flex, pipelined=True, **GUIDED)
    cat = [torch.cat([p[k] for p in parts]) for k in (0, 1)]
    print(f"[guidance] flex={flex}: slices vs whole {float((cat[0] - whole[0]).abs().max()):.3e} A, pipelined vs whole "
          f"{float((pipe[0] - whole[0]).abs().max()):.3e} A, pipelined vs slices {float((pipe[0] - cat[0]).abs().max()):.3e} A")
    assert torch.equal(pipe[0], cat[0]) and torch.equal(pipe[1], cat[1])
    assert torch.equal(cat[0], whole[0]) and torch.equal(cat[1], whole[1])
    assert torch.equal(pipe[0], whole[0]) and torch.equal(pipe[1], whole[1])


def test_t_max_below_every_t_equals_the_unguided_sampler_through_the_graph():
    plain = _run(steps=5, graph=True)
    off = _run(steps=5, graph=True, clash_guidance_weight=2.0, clash_guidance_t_max=0.0)
    guided = _run(steps=5, graph=True, **GUIDED)
    assert torch.equal(plain[0], off[0]) and torch.equal(plain[1], off[1])
    assert not torch.equal(plain[0], guided[0])
