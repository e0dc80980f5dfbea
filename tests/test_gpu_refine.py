"""csrc/ddp_refine.hip on the device: ddp_refine_energy against the fp64 statement of the energy on the same fp32 inputs (every
lane-stride edge of the receptor loop, the atom limit, shared and per-sample receptors), ddp_refine_direction against the CPU form,
ddp_refine_accept on hand-made energies, one full iteration against the CPU form, and PoseRefiner.refine on device tensors with the
invariants of tests/test_refine_cpu.py."""
import numpy as np
import pytest
import torch

from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd.sampler import modify_conformer, modify_conformer_hip
from test_refine_cpu import _CACHE, check_invariants, mild_cpu_run, mild_fixture, synthetic_case

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def statement(x, anchor, lig_r, rec, rec_r, pairs, overlap, k):
    """The energy's definition in fp64 PyTorch on the tensors' device, sample by sample, with every pair term kept apart:
    (energy [S, 4], grad [S, n, 3], sum of |energy terms| [S, 4], sum of |gradient terms| [S, n, 3])."""
    S, n = x.shape[0], x.shape[1]
    dev = x.device
    r = lig_r.double()
    e, ae = torch.zeros(S, 4, dtype=torch.float64, device=dev), torch.zeros(S, 4, dtype=torch.float64, device=dev)
    g, ag = torch.zeros(S, n, 3, dtype=torch.float64, device=dev), torch.zeros(S, n, 3, dtype=torch.float64, device=dev)

    def terms(diff, t, ok):
        d = diff.pow(2).sum(-1).sqrt()
        pen = torch.where(ok, (t - d).clamp(min=0), torch.zeros_like(d))
        unit = torch.where((d > 0)[..., None], diff / d[..., None], torch.zeros_like(diff))
        return pen.pow(2), (-2.0 * pen)[..., None] * unit

    t_c = r[:, None] + rec_r.double()[None] - 2.0 * overlap
    ok_c = (rec_r[None] >= 0) & (t_c > 0)
    t_s = r[:, None] + r[None] - 2.0 * overlap
    ok_s = ((pairs | pairs.T).bool() & (t_s > 0)) if pairs is not None else None
    for s in range(S):
        xs = x[s].double()
        if rec.shape[-2] > 0:
            rs = (rec[s] if rec.dim() == 3 else rec).double()
            pe, pg = terms(xs[:, None] - rs[None], t_c, ok_c)
            e[s, 0] = ae[s, 0] = pe.sum()
            g[s] += pg.sum(1)
            ag[s] += pg.abs().sum(1)
        if ok_s is not None:
            pe, pg = terms(xs[:, None] - xs[None], t_s, ok_s)
            e[s, 1] = ae[s, 1] = 0.5 * pe.sum()
            g[s] += pg.sum(1)
            ag[s] += pg.abs().sum(1)
        dx = xs - anchor[s].double()
        e[s, 2] = ae[s, 2] = k * dx.pow(2).sum(-1).mean()
        g[s] += (2.0 * k / n) * dx
        ag[s] += ((2.0 * k / n) * dx).abs()
    e[:, 3], ae[:, 3] = e[:, :3].sum(1), ae[:, :3].sum(1)
    return e, g, ae, ag


def _energy_launch(x, anchor, lig_r, rec, rec_r, pairs, overlap, k, with_grad=True):
    S, n = x.shape[0], x.shape[1]
    e = torch.full((S, 4), -7.0, dtype=torch.float64, device=x.device)
    g = torch.full((S, n, 3), -7.0, dtype=torch.float64, device=x.device) if with_grad else None
    LA.refine_energy(LA.refine_args(x, anchor, lig_r, rec, rec_r, pairs, overlap, k, e, g))
    return e, g


def _check_energy(case, overlap=0.4, k=0.25):
    dev = _dev()
    x, anchor, lig_r, rec, rec_r, pairs = (t.to(dev) for t in case)
    e, g = _energy_launch(x, anchor, lig_r, rec, rec_r, pairs, overlap, k)
    want_e, want_g, ae, ag = statement(x, anchor, lig_r, rec, rec_r, pairs, overlap, k)
    # both sides are fp64: only the order of summation differs, at most 2^20 2^10 terms of 2^-53 relative each -> 1e-9 sum |terms|
    err_e, err_g = (e - want_e).abs(), (g - want_g).abs()
    assert bool((err_e <= 1e-9 * ae).all()), (tuple(x.shape), tuple(rec.shape), float((err_e / ae.clamp(min=1e-300)).max()))
    assert bool((err_g <= 1e-9 * ag).all()), (tuple(x.shape), tuple(rec.shape), float((err_g / ag.clamp(min=1e-300)).max()))
    e2, g2 = _energy_launch(x, anchor, lig_r, rec, rec_r, pairs, overlap, k)
    assert torch.equal(_bits(e), _bits(e2)) and torch.equal(_bits(g), _bits(g2)), "two launches differ"
    return e, want_e


@pytest.mark.parametrize("n", [1, 4, 37, 300, 1024])
def test_energy_matches_the_fp64_statement(n):
    hit_cross = hit_self = False
    for S in (1, 3, 16):
        for m in (0, 1, 255, 256, 257, 2463):
            for per_sample in (False, True):
                e, want = _check_energy(synthetic_case(S, n, m, seed=1000 * S + m + n, per_sample_rec=per_sample))
                hit_cross |= bool((want[:, 0] > 0).any())
                hit_self |= bool((want[:, 1] > 0).any())
                if m == 0:
                    assert bool((e[:, 0] == 0).all())
    assert hit_cross and (hit_self or n < 37)          # the cases do hold overlapping pairs
    torch.cuda.synchronize()


def test_energy_without_a_positive_threshold_without_pairs_and_without_a_gradient():
    dev = _dev()
    e, want = _check_energy(synthetic_case(3, 37, 257, seed=9, all_far=True), k=0.0)
    assert torch.equal(e, torch.zeros_like(e))
    x, anchor, lig_r, rec, rec_r, pairs = (t.to(dev) for t in synthetic_case(3, 37, 257, seed=10))
    full, g = _energy_launch(x, anchor, lig_r, rec, rec_r, pairs, 0.4, 0.25)
    nogr, none = _energy_launch(x, anchor, lig_r, rec, rec_r, pairs, 0.4, 0.25, with_grad=False)
    assert none is None and torch.equal(_bits(full), _bits(nogr))
    nosp, _ = _energy_launch(x, anchor, lig_r, rec, rec_r, None, 0.4, 0.25)
    assert torch.equal(nosp[:, 1], torch.zeros(3, dtype=torch.float64, device=dev)) and torch.equal(_bits(nosp[:, 0]), _bits(full[:, 0]))
    # another overlap: the threshold moves
    _check_energy(synthetic_case(2, 37, 257, seed=11), overlap=0.1, k=1.5)
    # a NaN coordinate poisons its own sample only
    x2 = x.clone()
    x2[1, 3, 0] = float("nan")
    en, _ = _energy_launch(x2, anchor, lig_r, rec, rec_r, pairs, 0.4, 0.25)
    assert bool(torch.isnan(en[1, 3])) and torch.equal(_bits(en[0]), _bits(full[0])) and torch.equal(_bits(en[2]), _bits(full[2]))
    torch.cuda.synchronize()


def test_limits_and_empty_calls():
    dev = _dev()
    n = L.DDP_EVAL_MAX_ATOMS + 1
    x = torch.zeros(2, n, 3, device=dev)
    e = torch.zeros(2, 4, dtype=torch.float64, device=dev)
    args = LA.refine_args(x, x, torch.ones(n, device=dev), torch.zeros(5, 3, device=dev), torch.ones(5, device=dev), energy=e)
    assert L.load().ddp_refine_energy(args, LA.stream()) == -2          # DDP_ELIMIT
    with pytest.raises(L.DdpError, match="DDP_EVAL_MAX_ATOMS"):
        LA.refine_energy(args)
    # S = 0: nothing is launched, nothing is written
    x0 = torch.zeros(0, 5, 3, device=dev)
    LA.refine_energy(LA.refine_args(x0, x0, torch.ones(5, device=dev), torch.zeros(5, 3, device=dev), torch.ones(5, device=dev),
                                    energy=torch.zeros(0, 4, dtype=torch.float64, device=dev)))
    # index tables are checked on the host
    x5 = torch.zeros(1, 5, 3, device=dev)
    for bad in ([[0, 5]], [[-1, 2]]):
        with pytest.raises(L.DdpError, match="bonds"):
            LA.refine_bonds(torch.tensor(bad), 5, dev)
    with pytest.raises(L.DdpError, match="host"):                      # a device table is not downloaded to be looked at
        LA.refine_bonds(torch.tensor([[0, 1]], device=dev), 5, dev)
    ok = LA.refine_bonds(torch.tensor([[0, 4], [3, 1]]), 5, dev)
    assert ok.is_cuda and ok.dtype == torch.int32 and ok.cpu().tolist() == [[0, 4], [3, 1]]
    assert LA.refine_bonds(torch.zeros(0, 2, dtype=torch.long), 5, dev).shape == (0, 2)
    with pytest.raises(L.DdpError, match="self_pairs"):
        LA.refine_args(x5, x5, torch.ones(5, device=dev), torch.zeros(0, 3, device=dev), torch.ones(0, device=dev),
                       self_pairs=torch.zeros(4, 4, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- direction
def _check_direction(x, g, bonds, mask, step):
    dev = _dev()
    S, n, T = x.shape[0], x.shape[1], bonds.shape[0]
    tr, rot = torch.full((S, 3), -7.0, device=dev), torch.full((S, 3), -7.0, device=dev)
    tor = torch.full((S, T), -7.0, device=dev)
    xd = x.to(dev)
    args = LA.refine_args(xd, xd, torch.ones(n, device=dev), torch.zeros(0, 3, device=dev), torch.ones(0, device=dev), grad=g.to(dev),
                          bonds=LA.refine_bonds(bonds, n, dev), mask_rotate=mask.to(torch.uint8).to(dev), step=step.to(dev), tr=tr, rot=rot,
                          tor=tor)
    LA.refine_direction(args)
    want = [(step[:, None] * d) for d in R.direction_torch(x, g, bonds, mask)]
    for name, got, w in zip(("tr", "rot", "tor"), (tr, rot, tor), want):
        got = got.cpu().double()
        # the fp32 rounding of an fp64 result: relative 1e-6, absolute floor 1e-7 of the largest component
        bound = 1e-6 * w.abs() + 1e-7 * (float(w.abs().max()) if w.numel() else 0.0)
        assert bool(((got - w).abs() <= bound).all()), (name, n, T, float((got - w).abs().max()))
    return tr.cpu(), rot.cpu(), tor.cpu()


@pytest.mark.parametrize("T", [0, 1, 5])
def test_direction_matches_the_cpu_form(T):
    for n in (12, 300):
        gen = torch.Generator().manual_seed(10 * T + n)
        x = (torch.randn(3, n, 3, generator=gen) * 3).contiguous()
        g = torch.randn(3, n, 3, generator=gen, dtype=torch.float64)
        bonds = torch.stack([torch.randperm(n, generator=gen)[:2] for _ in range(T)]) if T else torch.zeros(0, 2, dtype=torch.long)
        mask = torch.rand(T, n, generator=gen) < 0.4
        if T:      # the last bond turns one atom only, and that atom is the bond's own end: on the axis, zero inertia
            mask[-1] = False
            mask[-1, bonds[-1, 0]] = True
        step = torch.tensor([1.0, 0.125, 768.0], dtype=torch.float64)
        tr, rot, tor = _check_direction(x, g, bonds, mask, step)
        if T:
            assert tor[:, -1].tolist() == [0.0, 0.0, 0.0]
    torch.cuda.synchronize()


def test_direction_of_one_atom_and_on_the_mild_fixture():
    x = torch.tensor([[[1.0, 2.0, 3.0]], [[-4.0, 0.5, 0.0]]])
    g = torch.tensor([[[0.5, -1.0, 2.0]], [[3.0, 0.0, -0.25]]], dtype=torch.float64)
    tr, rot, tor = _check_direction(x, g, torch.zeros(0, 2, dtype=torch.long), torch.zeros(0, 1, dtype=torch.bool),
                                    torch.tensor([2.0, 0.5], dtype=torch.float64))
    assert rot.tolist() == [[0.0] * 3] * 2 and tr.tolist() == [[-1.0, 2.0, -4.0], [-1.5, 0.0, 0.125]]
    rf, xm = mild_fixture()
    _, gm = rf.energy(xm)
    _check_direction(xm, gm, rf.bonds, rf.mask_rotate, torch.linspace(0.25, 4.0, 16, dtype=torch.float64))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- accept
@pytest.mark.parametrize("with_grad", [True, False])
def test_accept_on_hand_made_energies(with_grad):
    dev = _dev()
    nan = float("nan")
    S, n = 7, 70
    gen = torch.Generator().manual_seed(3)
    cur_tot = [5.0, 5.0, 5.0, 5.0, 5.0, 5.0, nan]
    tri_tot = [4.0, 5.0, 6.0, nan, np.nextafter(5.0, 0.0), 1.0, 1.0]
    take = [True, False, False, False, True, True, False]
    step0 = [1.0, 1.0, 3.0, 0.5, 600.0, 1024.0, 8.0]
    step1 = [2.0, 0.5, 1.5, 0.25, 1024.0, 1024.0, 4.0]
    e = torch.rand(S, 4, generator=gen, dtype=torch.float64)
    et = torch.rand(S, 4, generator=gen, dtype=torch.float64)
    e[:, 3], et[:, 3] = torch.tensor(cur_tot, dtype=torch.float64), torch.tensor(tri_tot, dtype=torch.float64)
    x, xt = torch.randn(S, n, 3, generator=gen), torch.randn(S, n, 3, generator=gen)
    g, gt = torch.randn(S, n, 3, generator=gen, dtype=torch.float64), torch.randn(S, n, 3, generator=gen, dtype=torch.float64)
    xt[3, 0, 0] = nan
    acc0 = torch.tensor([0, 3, 0, 0, 7, 1, 2], dtype=torch.int32)
    d = dict(x=x, xt=xt, e=e, et=et, g=g, gt=gt, step=torch.tensor(step0, dtype=torch.float64), acc=acc0)
    d = {k: v.clone().to(dev) for k, v in d.items()}
    args = LA.refine_args(d["x"], d["x"], torch.ones(n, device=dev), torch.zeros(0, 3, device=dev), torch.ones(0, device=dev),
                          energy=d["e"], grad=d["g"] if with_grad else None, step=d["step"], trial=d["xt"], trial_energy=d["et"],
                          trial_grad=d["gt"] if with_grad else None, accepted=d["acc"], grow=2.0, shrink=0.5, step_max=1024.0)
    LA.refine_accept(args)
    for s in range(S):
        src_x, src_e, src_g = (xt, et, gt) if take[s] else (x, e, g)
        assert torch.equal(_bits(d["x"][s].cpu()), _bits(src_x[s])), s
        assert torch.equal(_bits(d["e"][s].cpu()), _bits(src_e[s])), s
        assert torch.equal(_bits(d["g"][s].cpu()), _bits(src_g[s] if with_grad else g[s])), s
    assert d["step"].cpu().tolist() == step1
    assert d["acc"].cpu().tolist() == [int(a) + int(t) for a, t in zip(acc0.tolist(), take)]
    # the trial side is read only
    assert torch.equal(_bits(d["xt"].cpu()), _bits(xt)) and torch.equal(_bits(d["et"].cpu()), _bits(et))
    # other constants
    step = torch.full((S,), 2.0, dtype=torch.float64, device=dev)
    args.step, args.grow, args.shrink, args.step_max = step.data_ptr(), 3.0, 0.25, 5.0
    d["e"].copy_(e.to(dev))
    LA.refine_accept(args)
    assert step.cpu().tolist() == [5.0 if t else 0.5 for t in take]
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- one iteration, and the refiner
def _device_refiner(config=None):
    mild_fixture()
    return R.PoseRefiner(_CACHE["g"], _dev(), receptor=_CACHE["rec"], config=config)


def test_one_iteration_matches_the_cpu_form():
    dev = _dev()
    rf, x = mild_fixture()
    t = rf.evaluator._cpu
    S, n, T = x.shape[0], rf.n, rf.T

    def E(p):
        return R.energy_torch(p, x, t["lig_r"], t["rec"], t["rec_r"], rf.self_pairs, rf.overlap, 0.1)

    e, g = E(x)
    step = torch.ones(S, dtype=torch.float64)
    tr, rot, tor = ((step[:, None] * d).float() for d in R.direction_torch(x, g, rf.bonds, rf.mask_rotate))
    trial = modify_conformer(x, tr, rot, tor, rf.bonds, rf.rot_idx)
    et, _ = E(trial)
    take = et[:, 3] < e[:, 3]
    # the samples' decisions are clear of rounding: |E_trial - E| > 1e-6 E on every one of them
    assert bool(((et[:, 3] - e[:, 3]).abs() > 1e-6 * e[:, 3]).all())
    assert bool(take.any())

    rd = _device_refiner(R.RefineConfig(restraint=0.1))
    td = rd.evaluator._dev
    xd = x.to(dev)
    cur = xd.clone()
    f64 = dict(dtype=torch.float64, device=dev)
    ed, etd, gd, gtd = torch.empty(S, 4, **f64), torch.empty(S, 4, **f64), torch.empty(S, n, 3, **f64), torch.empty(S, n, 3, **f64)
    stepd, acc = torch.ones(S, **f64), torch.zeros(S, dtype=torch.int32, device=dev)
    trd, rotd, tord = torch.empty(S, 3, device=dev), torch.empty(S, 3, device=dev), torch.empty(S, T, device=dev)
    common = dict(lig_radii=td["lig_r"], rec=td["rec"], rec_radii=td["rec_r"], self_pairs=rd._pairs_dev, overlap=rd.overlap, restraint=0.1)
    a_cur = LA.refine_args(cur, xd, energy=ed, grad=gd, bonds=rd._bonds_i32, mask_rotate=rd._mask_u8, step=stepd, tr=trd, rot=rotd,
                           tor=tord, accepted=acc, **common)
    LA.refine_energy(a_cur)
    LA.refine_direction(a_cur)
    trial_d = modify_conformer_hip(cur, trd, rotd, tord, rd._bonds_i32, rd._mask_u8)
    a_tri = LA.refine_args(trial_d, xd, energy=etd, grad=gtd, **common)
    LA.refine_energy(a_tri)
    a_acc = LA.refine_args(cur, xd, energy=ed, grad=gd, step=stepd, trial=trial_d, trial_energy=etd, trial_grad=gtd, accepted=acc, **common)
    e_before = ed.clone()
    LA.refine_accept(a_acc)
    # trial poses: the bound of the ddp_pose_update tests (2e-5 of the largest coordinate)
    assert float((trial_d.cpu().double() - trial.double()).abs().max()) < 2e-5 * float(trial.double().abs().max())
    np.testing.assert_allclose(e_before.cpu().numpy(), e.numpy(), rtol=1e-9, atol=1e-12)
    assert acc.cpu().tolist() == take.to(torch.int32).tolist()
    assert stepd.cpu().tolist() == [2.0 if k else 0.5 for k in take.tolist()]
    want_x = torch.where(take[:, None, None].to(dev), trial_d, xd)
    assert torch.equal(_bits(cur), _bits(want_x))
    torch.cuda.synchronize()


def test_refine_on_device_keeps_the_invariants():
    dev = _dev()
    rf, x = mild_fixture()
    rd = _device_refiner(R.RefineConfig(restraint=0.1))
    xd = x.to(dev)
    keep = xd.clone()
    hist = []
    res = rd.refine(xd, history=hist)
    assert torch.equal(_bits(xd), _bits(keep)), "the input tensor was modified"
    # nothing inside refine waits for the device: with PyTorch's synchronisation check armed, a second call goes through
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        unsynced = rd.refine(xd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(_bits(unsynced.lig_pos), _bits(res.lig_pos))
    assert res.lig_pos.is_cuda and res.lig_pos.dtype == torch.float32 and res.energy_after.dtype == torch.float64
    check_invariants(rd, x, res, torch.stack(hist))
    # the start is the CPU form's start; the final poses are NOT compared (one flipped accept changes the step sequence)
    cpu_res, _ = mild_cpu_run()
    np.testing.assert_allclose(res.energy_before.cpu().numpy(), cpu_res.energy_before.numpy(), rtol=1e-9, atol=1e-12)
    assert torch.equal(res.clashes_before.cpu(), cpu_res.clashes_before)
    assert torch.equal(res.clashes_after, rd.evaluator.evaluate(res.lig_pos).clashes)
    # two runs give the same bits
    again = rd.refine(xd)
    for a, b in zip((res.lig_pos, res.energy_after, res.accepted, res.rmsd_moved), (again.lig_pos, again.energy_after, again.accepted,
                                                                                    again.rmsd_moved)):
        assert torch.equal(_bits(a), _bits(b))
    torch.cuda.synchronize()


def test_refine_on_device_fixed_point_and_nan_containment():
    dev = _dev()
    rf, x = mild_fixture()
    rd = _device_refiner()
    ref = _CACHE["g"]["ligand"].pos.float()[None].contiguous().to(dev)
    res = rd.refine(ref)
    assert torch.equal(res.energy_before, torch.zeros(1, 4, dtype=torch.float64, device=dev))
    assert torch.equal(_bits(res.lig_pos), _bits(ref)) and res.accepted.tolist() == [0]
    assert rd.refine(ref[:0]).lig_pos.shape == (0, rd.n, 3)
    r6 = _device_refiner(R.RefineConfig(iterations=6))
    bad = x[:4].clone().to(dev)
    bad[2, 5, 1] = float("nan")
    got, clean = r6.refine(bad), r6.refine(x[:4].to(dev))
    assert torch.equal(_bits(got.lig_pos[2]), _bits(bad[2])) and int(got.accepted[2]) == 0 and bool(torch.isnan(got.energy_after[2, 3]))
    for s in (0, 1, 3):
        assert torch.equal(_bits(got.lig_pos[s]), _bits(clean.lig_pos[s])) and torch.equal(_bits(got.energy_after[s]), _bits(clean.energy_after[s]))
        assert int(got.accepted[s]) == int(clean.accepted[s])
    with pytest.raises(ValueError):
        rf.refine(bad)                                     # a CPU refiner does not take device poses
    torch.cuda.synchronize()


def test_flexible_graph_reads_each_samples_own_receptor():
    from diffdock_pocket_amd.synthetic import make_3dpf_complex
    dev = _dev()
    g = make_3dpf_complex(seed=0, flexible_sidechains=True, n_lig=12, n_rec=8)
    rd = R.PoseRefiner(g, dev, config=R.RefineConfig(iterations=4))
    rc = R.PoseRefiner(g, config=R.RefineConfig(iterations=4))
    S = 3
    lig = (g["ligand"].pos.float()[None].repeat(S, 1, 1) + 1.2).contiguous()
    apos = g["atom"].pos.float()[None].repeat(S, 1, 1).contiguous()
    t = rc.evaluator._cpu
    pen = (t["lig_r"][:, None] + t["rec_r"][None] - 0.8 - torch.cdist(lig[1], apos[1])).clamp(min=0) * (t["rec_r"][None] >= 0)
    row = int(pen.sum(0).argmax())                         # the atom node that overlaps the ligand most
    assert float(pen[:, row].sum()) > 0
    e0, _ = rd.energy(lig.to(dev), atom_pos=apos.to(dev))
    want0, _ = rc.energy(lig, atom_pos=apos)
    assert bool((want0[:, 0] > 0).all())
    np.testing.assert_allclose(e0.cpu().numpy(), want0.numpy(), rtol=1e-9, atol=1e-12)
    apos[1, row] += 30.0                                   # one atom of sample 1 leaves the pocket
    e1, _ = rd.energy(lig.to(dev), atom_pos=apos.to(dev))
    want1, _ = rc.energy(lig, atom_pos=apos)
    np.testing.assert_allclose(e1.cpu().numpy(), want1.numpy(), rtol=1e-9, atol=1e-12)
    assert torch.equal(_bits(e1[0]), _bits(e0[0])) and torch.equal(_bits(e1[2]), _bits(e0[2])) and float(e1[1, 0]) < float(e0[1, 0])
    res = rd.refine(lig.to(dev), atom_pos=apos.to(dev))
    assert bool((res.energy_after[:, 3] <= res.energy_before[:, 3]).all()) and torch.equal(_bits(res.energy_before), _bits(e1))
    assert not torch.equal(_bits(res.lig_pos[1]), _bits(res.lig_pos[0])) and torch.equal(_bits(res.lig_pos[2]), _bits(res.lig_pos[0]))
    torch.cuda.synchronize()
