"""csrc/ddp_minimize.hip on the device: ddp_pose_minimize with iterations = 0 against the NumPy fp64 restatement of tests/vinardo_ref.py
within the derived bound (wave-only cases, the edges of the 1024-atom receptor tile, more than one tile, n = 256, shared and per-sample
receptors, with and without self pairs); one iteration against the CPU form with accepts and rejects; resumability, determinism and
batch independence, bit for bit; a full 50-iteration run on the 3dpf fixture against the CPU form's drop; NaN containment;
per-sample receptors; the limits and the fall-back above them; run_csv on the device."""
import ctypes

import numpy as np
import pytest
import torch

import vinardo_ref as V
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import minimize as M
from diffdock_pocket_amd import refine as R
from diffdock_pocket_amd.sampler import modify_conformer
from test_minimize_cpu import bits32, chain_case, check_invariants, flexible_case, run_50, tiled_graph
from test_scoring_cpu import CFG, as_torch, fixture_3dpf, perturbed_poses

pytestmark = pytest.mark.gpu
TILE = 1024          # DDP_MZ_TILE of csrc/ddp_minimize.hip


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _raw(t, anchor, iterations, k=0.0, bonds=None, mask=None, step=None, acc=None, history=False, grad=True):
    """ddp_pose_minimize on CLONES of the device state (x, step, accepted); returns (x, step, acc, e_in, e_out, history, grad)."""
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs = t
    S, n, dev = x.shape[0], x.shape[1], x.device
    x = x.clone()
    step = torch.ones(S, dtype=torch.float64, device=dev) if step is None else step.clone()
    acc = torch.zeros(S, dtype=torch.int32, device=dev) if acc is None else acc.clone()
    e0 = torch.full((S, 4), -7.0, dtype=torch.float64, device=dev)
    e1 = torch.full((S, 4), -7.0, dtype=torch.float64, device=dev)
    h = torch.full((iterations + 1, S), -7.0, dtype=torch.float64, device=dev) if history else None
    g = torch.full((S, n, 3), -7.0, dtype=torch.float64, device=dev) if grad else None
    LA.pose_minimize(x, anchor, lig_r, lig_f, rec, rec_r, rec_f, CFG, pairs, bonds, mask, step, acc, e0, e1, iterations, restraint=k,
                     history=h, grad=g)
    return x, step, acc, e0, e1, h, g


# ---------------------------------------------------------------------------------------------- 1. iterations = 0 against the restatement
@pytest.mark.parametrize("m", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 37])
@pytest.mark.parametrize("n", [1, 4, 37, 256])
def test_zero_iterations_match_the_fp64_restatement(n, m):
    """energy_in (inter, intra, restraint term, E) and grad against vinardo_ref.score + the restraint in NumPy fp64.  Bounds: inter,
    intra and the score's gradient as vinardo_ref.bounds derives them (256 eps (P + 1) max(1, largest |pair term|)); the restraint term
    is a sum of 3 n terms k dx^2 / n and gets the same form with P = 3 n; E the sum of the three; a gradient component one more term,
    (2 k / n) dx.  random_case redraws until no pair lies within 1e-6 A of the cutoff."""
    dev, k = _dev(), 0.7
    worst_e = worst_g = 0.0
    for S, per_sample, with_pairs in ((1, False, True), (3, True, True), (3, False, False), (1, True, False)):
        t, ref = as_torch(V.random_case(S, n, m, 31 * n + m + 5 * S + with_pairs, per_sample, with_pairs))
        anchor = t[0] + 0.25 * torch.randn(t[0].shape, generator=torch.Generator().manual_seed(n + m))
        td = [None if a is None else a.to(dev) for a in t]
        x, step, acc, e0, e1, h, g = _raw(td, anchor.to(dev), 0, k, history=True)
        torch.cuda.synchronize()
        dx = t[0].double().numpy() - anchor.double().numpy()
        terms = k * dx ** 2 / n
        rest = terms.reshape(S, -1).sum(1)
        be, bg = V.bounds(ref)
        b_rest = 256.0 * V.EPS * (3 * n + 1.0) * np.maximum(1.0, terms.reshape(S, -1).max(1))
        want = np.stack([ref["energy"][:, 4], ref["energy"][:, 5], rest, ref["energy"][:, 4] + ref["energy"][:, 5] + rest], 1)
        bound = np.stack([be[:, 4], be[:, 5], b_rest, be[:, 4] + be[:, 5] + b_rest], 1)
        err = np.abs(e0.cpu().numpy() - want)
        worst_e = max(worst_e, float((err / bound).max()))
        assert (err <= bound).all(), (S, per_sample, with_pairs, err / bound)
        gw = ref["grad"] + (2 * k / n) * dx
        bgr = 256.0 * V.EPS * (ref["n_pairs_grad"] + 2.0) * np.maximum(1.0, np.maximum(ref["max_grad"], (2 * k / n) * np.abs(dx).reshape(S, -1).max(1)))
        errg = np.abs(g.cpu().numpy() - gw)
        worst_g = max(worst_g, float((errg / bgr[:, None, None]).max()))
        assert (errg <= bgr[:, None, None]).all(), (S, per_sample, with_pairs)
        # nothing but the outputs is written: the pose bit for bit, step and accepted as they were, energy_out = energy_in = history[0]
        assert torch.equal(bits32(x), bits32(td[0])) and torch.equal(step, torch.ones_like(step)) and int(acc.sum()) == 0
        assert torch.equal(_bits(e0), _bits(e1)) and torch.equal(_bits(h[0]), _bits(e0[:, 3]))
        if m == 0:
            assert torch.equal(e0[:, 0], torch.zeros(S, dtype=torch.float64, device=dev))
        if not with_pairs:
            assert torch.equal(e0[:, 1], torch.zeros(S, dtype=torch.float64, device=dev))
    print(f"n={n} m={m}: worst |err| / bound energy {worst_e:.3e}, gradient {worst_g:.3e}")


@pytest.mark.parametrize("with_pairs", [True, False])
@pytest.mark.parametrize("m", [0, 1, TILE + 1])
@pytest.mark.parametrize("n", [1, 5, 37, 256])
def test_zero_iterations_equal_ddp_pose_score_bit_for_bit(n, m, with_pairs):
    """Both entries evaluate the score through the one score_evaluate of csrc/ddp_pose_descent.h: with restraint 0 and iterations = 0,
    energy_in[:, 0:2] of ddp_pose_minimize are the bits of energy[:, 4:6] of ddp_pose_score (gradient variant, tor_divisor 1) on the
    same poses, and the two gradients are the same bits.  S = 3; n = 5 is one more than the waves, n = 256 the fused limit; m = no
    tile, one atom, one atom into the second tile; one untyped atom on either side wherever there is more than one."""
    dev = _dev()
    t, _ = as_torch(V.random_case(3, n, m, 53 * n + m + with_pairs, False, with_pairs))
    if n > 1:
        t[1][n // 2] = -1.0
    if m > 1:
        t[4][m // 2] = -1.0
    td = [None if a is None else a.to(dev) for a in t]
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs = td
    assert (pairs is None) == (not with_pairs)
    _, _, _, e0, _, _, g = _raw(td, x, 0, 0.0)
    e7, gs = LA.pose_score(x, lig_r, lig_f, rec, rec_r, rec_f, CFG, 1.0, pairs, with_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e0[:, 0:2]), _bits(e7[:, 4:6])), (e0[:, 0:2] - e7[:, 4:6]).abs().max()
    assert torch.equal(_bits(g), _bits(gs)), (g - gs).abs().max()
    assert bool(torch.isfinite(gs).all())


# ---------------------------------------------------------------------------------------------- 2. one iteration against the CPU form
@pytest.mark.parametrize("fused", [True, False])
def test_one_iteration_matches_the_cpu_form(fused):
    """Per-sample input steps 2^-3 ... 2^9 on the 16-pose fixture: accepts and rejects both occur, and every decision is clear of
    rounding on the CPU side.  Energies: energy_in against the CPU form's at rtol 1e-9; energy_out of a REJECTED pose likewise; the
    energy_out of an ACCEPTED pose is the energy of the device's own trial, whose fp32 coordinates differ from the CPU trial's in
    the last bits (the 2e-5 max|coordinate| bound below), so it is compared at rtol 1e-9 with the CPU form's energy OF THE RETURNED
    POSE, and only to first order (sum |grad| |dx|) with the CPU form's energy of its own trial."""
    dev = _dev()
    g, _, full = fixture_3dpf()
    x = perturbed_poses()
    cpu, gpu = M.PoseMinimizer(g, receptor=full), M.PoseMinimizer(g, dev, receptor=full)
    step = torch.pow(2.0, torch.linspace(-3, 9, 16, dtype=torch.float64))
    zero = torch.zeros(16, dtype=torch.int32)
    xc, sc, ac, e0c, e1c = cpu.advance(x, x, step, zero, 1)
    # the CPU trial and its energy, restated
    e, grad = cpu.energy(x)
    d_tr, d_rot, d_tor = R.direction_torch(x, grad, cpu.bonds, cpu.mask_rotate)
    trial = modify_conformer(x, (step[:, None] * d_tr).float(), (step[:, None] * d_rot).float(), (step[:, None] * d_tor).float(),
                             cpu.bonds, cpu.rot_idx)
    et, gt = cpu.energy(trial, anchor=x)
    assert bool(((et[:, 3] - e[:, 3]).abs() > 1e-6 * e[:, 3].abs()).all()), "a decision of the fixture is not clear of rounding"
    take = et[:, 3] < e[:, 3]
    assert torch.equal(take.to(torch.int32), ac) and 0 < int(take.sum()) < 16, take
    xd, sd, ad, e0d, e1d = gpu.advance(x.to(dev), x.to(dev), step.to(dev), zero.to(dev), 1, fused=fused)
    xd, sd, ad, e0d, e1d = xd.cpu(), sd.cpu(), ad.cpu(), e0d.cpu(), e1d.cpu()
    assert torch.equal(ad, ac) and torch.equal(sd, sc)
    assert torch.equal(bits32(xd[~take]), bits32(x[~take])), "a rejected pose changed"
    scale = float(trial.abs().max())
    worst = float((xd[take].double() - trial[take].double()).abs().max())
    print(f"fused={fused}: accepted {int(take.sum())} of 16, accepted poses off the CPU trial by {worst:.2e} (bound {2e-5 * scale:.2e})")
    assert worst <= 2e-5 * scale

    def close(a, b):
        return bool(((a - b).abs() <= 1e-9 * b.abs() + 1e-12).all())

    assert close(e0d, e0c) and close(e1d[~take], e1c[~take])
    e_ret, _ = cpu.energy(xd, anchor=x)
    assert close(e1d, e_ret), float(((e1d - e_ret).abs() / e_ret.abs().clamp(min=1e-3)).max())
    first_order = (gt[take].abs().sum((1, 2)) * worst * 2.0)
    assert bool(((e1d[take, 3] - e1c[take, 3]).abs() <= 1e-9 * e1c[take, 3].abs() + first_order).all())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3. resumable, deterministic, independent
@pytest.mark.parametrize("n", [12, 37])
@pytest.mark.parametrize("T", [0, 1, 5])
def test_split_calls_and_repeated_launches_give_the_same_bits(T, n):
    dev = _dev()
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask = (a.to(dev) for a in chain_case(3, n, T, 300, 40 + T + n))
    t = [x, lig_r, lig_f, rec, rec_r, rec_f, pairs]
    kw = dict(k=0.1, bonds=bonds if T else None, mask=mask if T else None)
    whole = _raw(t, x, 12, history=True, **kw)
    again = _raw(t, x, 12, history=True, **kw)

    def same(a, b, what):
        assert torch.equal(bits32(a[0]), bits32(b[0])), what + ": pos"
        assert torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(a[2], b[2]), what + ": step / accepted"
        assert torch.equal(_bits(a[4]), _bits(b[4])), what + ": energy_out"

    same(whole, again, "two launches")
    assert torch.equal(_bits(whole[5]), _bits(again[5])) and torch.equal(_bits(whole[6]), _bits(again[6]))
    a = _raw(t, x, 5, **kw)
    b = _raw([a[0]] + t[1:], x, 7, step=a[1], acc=a[2], **kw)
    same(whole, b, "5 + 7")
    assert torch.equal(_bits(b[3]), _bits(a[4])) and torch.equal(_bits(whole[3]), _bits(a[3]))
    assert torch.equal(_bits(whole[6]), _bits(b[6])), "5 + 7: gradient at exit"
    cur = (x, None, None)
    hist = []
    for i in range(12):
        cur = _raw([cur[0]] + t[1:], x, 1, step=cur[1], acc=cur[2], history=True, **kw)
        hist.append(cur[5][1])
    same(whole, cur, "12 x 1")
    assert torch.equal(_bits(torch.stack(hist)), _bits(whole[5][1:]))
    h = whole[5]
    assert bool((h[1:] <= h[:-1]).all()) and int(whole[2].sum()) >= 1 and bool((whole[2] <= 12).all())
    print(f"T={T} n={n}: accepted {whole[2].tolist()}, E {h[0].tolist()} -> {h[-1].tolist()}")
    torch.cuda.synchronize()


def test_a_row_of_a_batch_equals_the_one_pose_launch():
    dev = _dev()
    g, _, full = fixture_3dpf()
    mz = M.PoseMinimizer(g, dev, receptor=full, config=M.MinimizeConfig(iterations=12))
    x = perturbed_poses().to(dev)
    batch = mz.minimize(x)
    again = mz.minimize(x)
    assert torch.equal(bits32(batch.lig_pos), bits32(again.lig_pos)) and torch.equal(_bits(batch.energy_after), _bits(again.energy_after))
    for s in range(16):
        one = mz.minimize(x[s:s + 1])
        assert torch.equal(bits32(one.lig_pos[0]), bits32(batch.lig_pos[s])) and torch.equal(_bits(one.energy_after[0]), _bits(batch.energy_after[s]))
        assert int(one.accepted[0]) == int(batch.accepted[s])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. a full run on the fixture
def test_a_full_run_on_the_fixture_recovers_the_cpu_forms_drop():
    """fused=True, 50 iterations: the invariants of the CPU file; a second call with the synchronisation debug mode armed;
    energy_after against an independent PoseScorer.score of the returned poses within the derived bound; per pose at least 95 % of
    the CPU form's drop.  Final poses of the two forms are not compared: one flipped accept changes the step sequence."""
    dev = _dev()
    g, _, full = fixture_3dpf()
    cpu_res, _ = run_50()
    mz = M.PoseMinimizer(g, dev, receptor=full, config=M.MinimizeConfig(iterations=50))
    x0 = perturbed_poses()
    xd = x0.to(dev)
    h = []
    res = mz.minimize(xd, history=h)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x0) and res.lig_pos.is_cuda and res.energy_after.is_cuda
    torch.cuda.set_sync_debug_mode("error")
    try:
        res2 = mz.minimize(xd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(bits32(res2.lig_pos), bits32(res.lig_pos))
    host = res.cpu()
    check_invariants(host, torch.stack(h).cpu(), x0, "device form, fused, 50 iterations")
    # energy_after against an independent score of the returned poses
    sc = mz.scorer.score(res.lig_pos).cpu()
    t = mz.scorer._cpu
    ref = V.score(host.lig_pos.numpy(), t["lig_r"].numpy(), t["lig_f"].numpy(), t["rec"].numpy(), t["rec_r"].numpy(), t["rec_f"].numpy(),
                  t["pairs"].numpy(), mz.scorer.tor_divisor)
    be, _ = V.bounds(ref)
    assert (np.abs(host.energy_after[:, 0].numpy() - sc.inter.numpy()) <= be[:, 4]).all()
    assert (np.abs(host.energy_after[:, 1].numpy() - sc.intra.numpy()) <= be[:, 5]).all()
    assert (np.abs(host.energy_after[:, 3].numpy() - (sc.inter + sc.intra).numpy()) <= be[:, 4] + be[:, 5]).all()
    assert torch.equal(host.energy_after[:, 2], torch.zeros(16, dtype=torch.float64))
    # at least 95 % of the CPU form's drop, per pose
    eb, ea, ec = host.energy_before[:, 3], host.energy_after[:, 3], cpu_res.energy_after[:, 3]
    ratio = (ea - ec) / (eb - ec)
    print("device E_after - CPU E_after, as a fraction of the CPU drop: worst", float(ratio.max()), "all", [round(float(v), 5) for v in ratio])
    assert bool((ea <= ec + 0.05 * (eb - ec)).all())


# ---------------------------------------------------------------------------------------------- 5. NaN, per-sample receptors
@pytest.mark.parametrize("fused", [True, False])
def test_a_nan_pose_is_kept_bit_for_bit_on_the_device(fused):
    dev = _dev()
    g, _, full = fixture_3dpf()
    mz = M.PoseMinimizer(g, dev, receptor=full, config=M.MinimizeConfig(iterations=6))
    x = perturbed_poses()[:4].to(dev)
    clean = mz.minimize(x, fused=fused)
    bad = x.clone()
    bad[2, 5, 1] = float("nan")
    got = mz.minimize(bad, fused=fused)
    torch.cuda.synchronize()
    assert torch.equal(bits32(got.lig_pos[2]), bits32(bad[2])) and int(got.accepted[2]) == 0
    assert bool(torch.isnan(got.energy_before[2, 3])) and bool(torch.isnan(got.energy_after[2, 3]))
    for s in (0, 1, 3):
        assert torch.equal(bits32(got.lig_pos[s]), bits32(clean.lig_pos[s])) and torch.equal(_bits(got.energy_after[s]), _bits(clean.energy_after[s]))
        assert int(got.accepted[s]) == int(clean.accepted[s]) >= 1


def test_flexible_graph_minimises_each_sample_against_its_own_atoms_on_the_device():
    dev = _dev()
    g, lig, apos, row = flexible_case()
    mz = M.PoseMinimizer(g, dev, config=M.MinimizeConfig(iterations=5))
    lig, apos = lig.to(dev), apos.to(dev)
    base = mz.minimize(lig, atom_pos=apos)
    assert torch.equal(bits32(base.lig_pos), bits32(mz.minimize(lig).lig_pos))
    moved = apos.clone()
    moved[1, row] += 30.0
    got = mz.minimize(lig, atom_pos=moved)
    torch.cuda.synchronize()
    for s in (0, 2):
        assert torch.equal(bits32(got.lig_pos[s]), bits32(base.lig_pos[s])) and torch.equal(_bits(got.energy_after[s]), _bits(base.energy_after[s]))
    assert not torch.equal(got.energy_before[1], base.energy_before[1])
    # and the device energies are the CPU form's on the same inputs
    e_cpu, _ = M.PoseMinimizer(g).energy(lig.cpu(), atom_pos=moved.cpu())
    assert torch.allclose(got.energy_before.cpu(), e_cpu, rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------------------------- 6. limits
def test_limits_return_codes_and_the_fall_back():
    dev = _dev()
    lib = L.load()
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs, bonds, mask = (a.to(dev) for a in chain_case(2, 8, 1, 5, 3))
    step, acc = torch.ones(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    e0 = torch.full((2, 4), -7.0, dtype=torch.float64, device=dev)
    e1 = torch.full((2, 4), -7.0, dtype=torch.float64, device=dev)
    pos = x.clone()

    def rc(**kw):
        a = L.MinimizeArgs(n_samples=2, n=8, m=5, rec_stride=0, n_tor=1, iterations=2, pos=pos.data_ptr(), anchor=x.data_ptr(),
                           lig_radii=lig_r.data_ptr(), lig_flags=lig_f.data_ptr(), rec=rec.data_ptr(), rec_radii=rec_r.data_ptr(),
                           rec_flags=rec_f.data_ptr(), self_pairs=pairs.data_ptr(), bonds=bonds.data_ptr(), mask_rotate=mask.data_ptr(),
                           cutoff=8.0, gauss_offset=0.0, gauss_width=0.8, hydrophobic_good=0.0, hydrophobic_bad=2.5, hbond_good=-0.6,
                           hbond_bad=0.0, w_gauss=-0.045, w_repulsion=0.8, w_hydrophobic=-0.035, w_hbond=-0.6, restraint=0.0, grow=2.0,
                           shrink=0.5, step_max=1024.0, step=step.data_ptr(), accepted=acc.data_ptr(), energy_in=e0.data_ptr(),
                           energy_out=e1.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ddp_pose_minimize(ctypes.byref(a), LA.stream())

    assert rc(n=L.DDP_MINIMIZE_MAX_ATOMS + 1) == -2 and rc(n_tor=L.DDP_MINIMIZE_MAX_TORSIONS + 1) == -2             # DDP_ELIMIT
    for bad in (dict(pos=None), dict(anchor=None), dict(lig_radii=None), dict(lig_flags=None), dict(step=None), dict(accepted=None),
                dict(energy_in=None), dict(energy_out=None), dict(rec=None), dict(rec_radii=None), dict(rec_flags=None), dict(bonds=None),
                dict(mask_rotate=None), dict(cutoff=0.0), dict(cutoff=float("nan")), dict(n_samples=-1), dict(n=0), dict(m=-1), dict(n_tor=-1),
                dict(rec_stride=14), dict(gauss_width=0.0), dict(hbond_bad=-0.6), dict(iterations=-1), dict(restraint=-0.1),
                dict(restraint=float("nan"))):
        assert rc(**bad) == -1, bad                                                                                   # DDP_EINVAL
    assert rc(n_samples=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(e0, torch.full_like(e0, -7.0)) and torch.equal(bits32(pos), bits32(x)), "a guard launched"
    assert rc() == 0 and rc(m=0, rec=None, rec_radii=None, rec_flags=None, n_tor=0, bonds=None, mask_rotate=None, self_pairs=None) == 0
    torch.cuda.synchronize()
    assert bool((e0 != -7.0).all()) and bool((e1 != -7.0).all())
    with pytest.raises(L.DdpError, match="DDP_MINIMIZE_MAX_ATOMS"):
        big = torch.zeros(1, L.DDP_MINIMIZE_MAX_ATOMS + 1, 3, device=dev)
        nb = big.shape[1]
        LA.pose_minimize(big, big.clone(), torch.ones(nb, device=dev), torch.zeros(nb, dtype=torch.uint8, device=dev), rec, rec_r, rec_f, CFG,
                         None, None, None, step[:1].clone(), acc[:1].clone(), e0[:1].clone(), e1[:1].clone(), 1)
    with pytest.raises(L.DdpError, match="step"):
        LA.pose_minimize(pos, x, lig_r, lig_f, rec, rec_r, rec_f, CFG, pairs, bonds, mask, step.float(), acc, e0, e1, 1)
    # a ligand above the limit: fused=True falls back to the launch-by-launch path, with a warning that names the limit
    copies = L.DDP_MINIMIZE_MAX_ATOMS // 37 + 1
    big_g = tiled_graph(copies)
    mz = M.PoseMinimizer(big_g, dev, config=M.MinimizeConfig(iterations=3))
    assert mz.n == 37 * copies > L.DDP_MINIMIZE_MAX_ATOMS and not mz.fused_available()
    poses = (big_g["ligand"].pos.float()[None] + 0.2 * torch.randn(2, mz.n, 3, generator=torch.Generator().manual_seed(1))).to(dev)
    M._warned.clear()
    with pytest.warns(UserWarning, match="DDP_MINIMIZE_MAX_ATOMS"):
        fell = mz.minimize(poses, fused=True)
    slow = mz.minimize(poses, fused=False)
    torch.cuda.synchronize()
    assert torch.equal(bits32(fell.lig_pos), bits32(slow.lig_pos)) and torch.equal(_bits(fell.energy_after), _bits(slow.energy_after))
    assert torch.equal(fell.accepted, slow.accepted) and int(slow.accepted.sum()) >= 1


# ---------------------------------------------------------------------------------------------- 7. the driver on the device
def test_run_csv_minimises_on_the_device(tmp_path):
    import os
    from test_gpu_trajectory import GOLDEN, _model_dir
    dev = _dev()
    model_dir = _model_dir(tmp_path, False)
    model, margs, sigma = INF._load_model(model_dir, "best_ema_inference_epoch_model.pt", dev)
    pdb, sdf = os.path.join(GOLDEN, "3dpf_protein.pdb"), os.path.join(GOLDEN, "3dpf_ligand.sdf")
    csv_path = tmp_path / "one.csv"
    csv_path.write_text("complex_name,experimental_protein,ligand,pocket_center_x,pocket_center_y,pocket_center_z,flexible_sidechains\n"
                        f"3dpf,{pdb},{sdf},,,,\n")
    gk = {k: getattr(margs, k) for k in ("receptor_radius", "c_alpha_max_neighbors", "remove_hs", "pocket_reduction", "pocket_buffer",
                                         "pocket_cutoff")}
    from diffdock_pocket_amd.sampler import SamplerConfig
    cfg = SamplerConfig(inference_steps=4, sigma=sigma, flexible_sidechains=False)
    res = INF.run_csv(str(csv_path), model, dev, samples_per_complex=3, inference_steps=4, seed=7, sampler_cfg=cfg, graph_kwargs=gk,
                      allow_zero_esm=True, out_dir=str(tmp_path / "out"), minimize_poses=M.MinimizeConfig(iterations=3))[0]
    assert res.skipped is None, res.skipped
    mr = res.minimized
    assert isinstance(mr, M.MinimizeResult) and not mr.lig_pos.is_cuda and mr.lig_pos.shape == res.ligand_pos.shape
    assert torch.equal(mr.lig_pos, res.minimized_pos) and bool((mr.energy_after[:, 3] <= mr.energy_before[:, 3]).all())
    names = {os.path.basename(f) for f in res.files}
    assert {"minimized.csv", "rank1_minimized.sdf", "rank2_minimized.sdf", "rank3_minimized.sdf"} <= names
    assert names == set(os.listdir(os.path.dirname(res.files[0])))
    torch.cuda.synchronize()
