"""csrc/ddp_profile.hip on the device: ddp_pose_profile against the NumPy fp64 restatement of tests/interactions_ref.py on the same
fp32 inputs within the derived bound at the smallest shapes where the kernel can go wrong, bit reproducibility, the receptor stride,
the sum over the residues against ddp_pose_score, the poison rule, limits and return codes, the device InteractionProfiler against the
CPU one on the 3dpf fixture, and run_csv on the device with the stub model."""
import ctypes
import os

import numpy as np
import pytest
import torch

import interactions_ref as IR
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import interactions as IA
from diffdock_pocket_amd import launch as LA
from test_evaluation_cpu import graph_3dpf
from test_gpu_scoring import DeviceStub
from test_interactions_cpu import SHAPES, case, check_poison, check_profile, profile_3dpf
from test_scoring_cpu import CFG, CSV, GOLDEN, fixture_3dpf, perturbed_poses

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _launch(t, sentinel=-7.0):
    """ddp_pose_profile on the tensors t = (x, lig_r, lig_f, rec, rec_r, rec_f, res_ptr), moved to the device, into sentinel-filled
    outputs."""
    t = [a.to(_dev()) for a in t]
    S, R = t[0].shape[0], t[6].shape[0] - 1
    p = torch.full((S, R, 7), sentinel, dtype=torch.float64, device=_dev())
    b = torch.full((S, R), 0xEE, dtype=torch.uint8, device=_dev())
    LA.pose_profile(*t, CFG, 4.5, profile=p, bits=b)
    return p, b


# ---------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernel_matches_the_fp64_restatement(name):
    t, ref = case(name)
    p, b = _launch(t)
    check_profile(p, b, ref, name)            # (every entry is written: a sentinel left behind fails pairs, d_min and the bits)
    assert ref["threshold_gap"] >= 1e-6
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. reproducibility
def test_two_launches_and_batch_positions_give_the_same_bits():
    t, _ = case("ragged_90")
    p, b = _launch(t)
    p2, b2 = _launch(t)
    assert torch.equal(_bits(p), _bits(p2)) and torch.equal(b, b2), "two launches differ"
    # sample 0 at batch position 3, among different poses
    x = t[0]
    moved = torch.cat([x[1:2], x[2:3] + 1.0, x[3:4] - 2.0, x[0:1]], 0).contiguous()
    p3, b3 = _launch([moved] + t[1:])
    assert torch.equal(_bits(p3[3]), _bits(p[0])) and torch.equal(b3[3], b[0]) and torch.equal(_bits(p3[0]), _bits(p[1]))
    assert not torch.equal(_bits(p3[1]), _bits(p[2]))
    one = _launch([x[0:1].contiguous()] + t[1:])
    assert torch.equal(_bits(one[0][0]), _bits(p[0])) and torch.equal(one[1][0], b[0])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3. receptor stride
def test_per_sample_receptors_are_read_through_the_stride():
    t, ref = case("per_sample_receptors")
    p, b = _launch(t)
    check_profile(p, b, ref, "per-sample receptors")            # each sample against its own receptor
    assert not torch.equal(p[0], p[1])
    # one receptor replicated for every sample: stride 3 m and stride 0 give the same bits
    shared = t[3][1].contiguous()
    p_rep, b_rep = _launch(t[:3] + [shared[None].repeat(4, 1, 1).contiguous()] + t[4:])
    p_one, b_one = _launch(t[:3] + [shared] + t[4:])
    assert torch.equal(_bits(p_rep), _bits(p_one)) and torch.equal(b_rep, b_one) and torch.equal(_bits(p_rep[1]), _bits(p[1]))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. against ddp_pose_score
@pytest.mark.parametrize("name", ["ragged_90", "per_sample_receptors", "one_past_a_wave"])
def test_sum_over_the_residues_matches_ddp_pose_score(name):
    t, ref = case(name)
    p, _ = _launch(t)
    d = [a.to(_dev()) for a in t]
    e, _ = LA.pose_score(*d[:6], CFG, 1.0)
    bt, be = IR.bounds(ref)
    err_t = (p[..., :4].sum(1) - e[:, :4]).abs().cpu().numpy()
    err_e = (p[..., 4].sum(1) - e[:, 4]).abs().cpu().numpy()
    print(name, "sum over residues against ddp_pose_score: worst |err| / summed bound", float((err_t / bt.sum(1)).max()),
          float((err_e / be.sum(1)).max()))
    assert (err_t <= bt.sum(1)).all() and (err_e <= be.sum(1)).all() and float(e[:, 0].min()) > 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. the poison rule
def test_poison_rule_on_the_device():
    check_poison(_launch)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 6. limits and return codes
def test_limits_return_codes_and_empty_calls():
    dev = _dev()
    lib = L.load()
    t, _ = case("five_single_atom_residues")
    x, lig_r, lig_f, rec, rec_r, rec_f, ptr = [a.to(dev) for a in t]
    p = torch.full((4, 5, 7), -7.0, dtype=torch.float64, device=dev)
    b = torch.full((4, 5), 0xEE, dtype=torch.uint8, device=dev)

    def args(**kw):
        a = L.ProfileArgs(n_samples=4, n=3, m=5, rec_stride=0, n_res=5, pos=x.data_ptr(), lig_radii=lig_r.data_ptr(),
                          lig_flags=lig_f.data_ptr(), rec=rec.data_ptr(), rec_radii=rec_r.data_ptr(), rec_flags=rec_f.data_ptr(),
                          res_ptr=ptr.data_ptr(), cutoff=8.0, gauss_offset=0.0, gauss_width=0.8, hydrophobic_good=0.0, hydrophobic_bad=2.5,
                          hbond_good=-0.6, hbond_bad=0.0, w_gauss=-0.045, w_repulsion=0.8, w_hydrophobic=-0.035, w_hbond=-0.6,
                          contact_distance=4.5, profile=p.data_ptr(), bits=b.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rc(**kw):
        return lib.ddp_pose_profile(ctypes.byref(args(**kw)), LA.stream())

    assert rc(n=L.DDP_EVAL_MAX_ATOMS + 1) == -2                                                       # DDP_ELIMIT
    for bad in (dict(pos=None), dict(lig_radii=None), dict(lig_flags=None), dict(profile=None), dict(bits=None), dict(res_ptr=None),
                dict(rec=None), dict(rec_radii=None), dict(rec_flags=None), dict(cutoff=0.0), dict(cutoff=float("inf")),
                dict(cutoff=float("nan")), dict(n_samples=-1), dict(n=0), dict(n=-3), dict(m=-1), dict(n_res=-1), dict(rec_stride=14),
                dict(gauss_width=0.0), dict(hbond_bad=-0.6), dict(contact_distance=0.0), dict(contact_distance=float("nan"))):
        assert rc(**bad) == -1, bad                                                                   # DDP_EINVAL
    assert lib.ddp_pose_profile(None, LA.stream()) == -1
    with pytest.raises(L.DdpError, match="DDP_EVAL_MAX_ATOMS"):
        big = torch.zeros(1, L.DDP_EVAL_MAX_ATOMS + 1, 3, device=dev)
        LA.pose_profile(big, torch.ones(big.shape[1], device=dev), torch.zeros(big.shape[1], dtype=torch.uint8, device=dev), rec, rec_r,
                        rec_f, ptr, CFG)
    # nothing above launched; n_samples = 0 and n_res = 0 return 0 and launch nothing: the sentinel-filled outputs are untouched
    assert rc(n_samples=0) == 0 and rc(n_res=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(p, torch.full_like(p, -7.0)) and torch.equal(b, torch.full_like(b, 0xEE))
    assert LA.pose_profile(x[:0], lig_r, lig_f, rec, rec_r, rec_f, ptr, CFG)[0].shape == (0, 5, 7)
    assert LA.pose_profile(x, lig_r, lig_f, rec, rec_r, rec_f, ptr[:1], CFG)[1].shape == (4, 0)
    # m = 0 needs no receptor pointers (every residue is empty); a valid call does write
    empty = torch.zeros(6, dtype=torch.int32, device=dev)
    assert rc(m=0, rec=None, rec_radii=None, rec_flags=None, res_ptr=empty.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(p[..., :5], torch.zeros(4, 5, 5, dtype=torch.float64, device=dev)) and bool(torch.isinf(p[..., 5]).all())
    assert not p[..., 6].any() and not b.any()
    assert rc() == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(p), _bits(_launch(t)[0]))
    # shapes are checked on the host
    with pytest.raises(L.DdpError, match="res_ptr"):
        LA.pose_profile(x, lig_r, lig_f, rec, rec_r, rec_f, ptr.to(torch.int64), CFG)
    with pytest.raises(L.DdpError, match="lig_flags"):
        LA.pose_profile(x, lig_r, lig_f.to(torch.int32), rec, rec_r, rec_f, ptr, CFG)
    with pytest.raises(L.DdpError, match="rec"):
        LA.pose_profile(x, lig_r, lig_f, rec[None].repeat(3, 1, 1), rec_r, rec_f, ptr, CFG)
    with pytest.raises(L.DdpError, match="bits"):
        LA.pose_profile(x, lig_r, lig_f, rec, rec_r, rec_f, ptr, CFG, bits=torch.zeros(4, 4, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7. the profiler on the device
def _as_rows(out):
    return torch.cat([out.terms, out.energy[..., None], out.d_min[..., None], out.pairs.double()[..., None]], -1)


def _restate(pf, x, atom_pos=None):
    t = pf._cpu
    rec = t["rec"] if atom_pos is None else atom_pos[:, t["keep"]]
    return IR.profile(x.numpy(), t["lig_r"].numpy(), t["lig_f"].numpy(), rec.numpy(), t["rec_r"].numpy(), t["rec_f"].numpy(), t["ptr"].numpy())


def _check_both(gpu_out, cpu_out, ref):
    """Both forms within the bound of the restatement; the bits wherever the pose stays 1e-6 clear of every threshold, which at most
    one of the 16 poses may fail to."""
    clear = ref["gap"] >= 1e-6
    print("poses left out of the bit comparison:", int((~clear).sum()))
    assert int((~clear).sum()) <= 1
    for out, what in ((gpu_out.cpu(), "device"), (cpu_out, "host")):
        check_profile(_as_rows(out), out.bits, ref, what, bits_where=clear)
    assert torch.equal(gpu_out.cpu().bits[clear], cpu_out.bits[clear]) and torch.equal(gpu_out.cpu().pairs, cpu_out.pairs)


def test_device_profiler_matches_the_cpu_profiler_on_3dpf():
    dev = _dev()
    g, pdb, full = fixture_3dpf()
    x = perturbed_poses()
    table = IA.receptor_residues(pdb)
    for cpu, receptor in zip(profile_3dpf(), ((full, table), "graph")):
        gpu = IA.InteractionProfiler(g, dev, receptor=receptor)
        got = gpu.profile(x.to(dev))
        assert got.bits.is_cuda and got.terms.dtype == torch.float64 and got.terms.shape == (16, cpu.n_res, 4) and got.labels == cpu.labels
        _check_both(got, cpu.profile(x), _restate(cpu, x))
        assert got.similarity().is_cuda and got.similarity().shape == (16, 16) and got.frequency().shape == (cpu.n_res, 3)
        assert torch.equal(got.similarity().cpu(), got.cpu().similarity())
    with pytest.raises(ValueError):
        cpu.profile(x.to(dev))                                # a CPU profiler does not take device poses
    # the flexible graph with each sample's own atom positions
    gf, _ = graph_3dpf(flex="A:160-A:193-A:197")
    cpu, gpu = IA.InteractionProfiler(gf), IA.InteractionProfiler(gf, dev)
    gen = torch.Generator().manual_seed(4)
    apos = (gf["atom"].pos.float()[None] + 0.2 * torch.randn(16, cpu.n_a, 3, generator=gen)).contiguous()
    got = gpu.profile(x.to(dev), atom_pos=apos.to(dev))
    _check_both(got, cpu.profile(x, atom_pos=apos), _restate(cpu, x, apos))
    assert not torch.equal(got.energy[0], gpu.profile(x.to(dev)).energy[0])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 8. the driver on the device
def test_run_csv_on_the_device_matches_the_cpu_run(tmp_path):
    """As test_gpu_scoring does for the score: the sampler's arithmetic differs between the devices in the last fp32 bits of the poses,
    so each run's profile is checked against the restatement on ITS OWN poses within the bound, and the two runs' energies against
    each other within the bound plus what a pose difference of that size can move them: to first order |dE| <= dx sum over the
    residue's pairs of the 1-norm of the pair gradient (interactions_ref grad_l1), taken twice, plus the largest pair energy at the
    cutoff (0.045 exp(-((8 - 4.72) / 0.8)^2) < 3e-9) twice for every pair of the residue, which may cross it."""
    from test_inference_csv import StubConfidence
    dev = _dev()
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)

    def run(device, out):
        return INF.run_csv(str(p), DeviceStub(), device, confidence_model=StubConfidence(), samples_per_complex=4, inference_steps=2,
                           root=GOLDEN, seed=2, allow_zero_esm=True, out_dir=str(tmp_path / out), interaction_profile=IA.ProfileConfig())

    on_cpu, on_dev = run(torch.device("cpu"), "cpu"), run(dev, "dev")
    full_pf, _ = profile_3dpf()
    for k, (a, b) in enumerate(zip(on_cpu, on_dev)):
        assert a.skipped is None and b.skipped is None and not b.interactions.bits.is_cuda
        assert a.order.tolist() == b.order.tolist() and a.interactions.labels == b.interactions.labels
        assert sorted(os.path.basename(f) for f in a.files) == sorted(os.path.basename(f) for f in b.files)
        assert {"interactions.csv", "interaction_summary.csv", "interaction_similarity.csv"} <= {os.path.basename(f) for f in b.files}
        dx = float((a.ligand_pos.double() - b.ligand_pos.double()).abs().max())
        assert dx < 1e-3
        if k == 1:          # the rigid row: the full PDB receptor, the same on both devices
            refs = []
            for r in (a, b):
                ref = _restate(full_pf, r.ligand_pos)
                refs.append(ref)
                check_profile(_as_rows(r.interactions), r.interactions.bits, ref, "run_csv", bits_where=ref["gap"] >= 1e-6)
            be = IR.bounds(refs[0])[1] + IR.bounds(refs[1])[1]
            n_typed = int((full_pf._cpu["lig_r"] >= 0).sum())
            sizes = np.diff(full_pf._cpu["ptr"].numpy())[None]
            slack = 2.0 * dx * np.maximum(refs[0]["grad_l1"], refs[1]["grad_l1"]) + 2 * 3e-9 * n_typed * sizes
            diff = np.abs(a.interactions.energy.numpy() - b.interactions.energy.numpy())
            print("run_csv: largest energy difference", float(diff.max()), "of", float((be + slack).max()), "dx", dx)
            assert (diff <= be + slack).all()
    torch.cuda.synchronize()
