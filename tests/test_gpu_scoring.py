"""csrc/ddp_score.hip on the device: ddp_pose_score against the NumPy fp64 restatement of tests/vinardo_ref.py on the same fp32 inputs
within the derived bound (the first wave-only case, the edges of the 1024-atom receptor tile, more than one tile, the atom limit),
bit reproducibility, the receptor stride, limits and return codes, the device PoseScorer against the CPU one on the 3dpf fixture,
NaN containment, and run_csv on the device with the stub model."""
import ctypes

import numpy as np
import pytest
import torch

import vinardo_ref as V
from diffdock_pocket_amd import _lib as L
from diffdock_pocket_amd import inference as INF
from diffdock_pocket_amd import launch as LA
from diffdock_pocket_amd import scoring as SC
from test_evaluation_cpu import graph_3dpf
from test_scoring_cpu import CFG, CSV, GOLDEN, as_torch, check_against_ref, fixture_3dpf, perturbed_poses

pytestmark = pytest.mark.gpu
DIV = 1.0 + V.W_TORSION * 3          # the divisor vinardo_ref.random_case scores with


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int64)


def _launch(t, with_grad=True, with_pairs=True, sentinel=-7.0):
    """ddp_pose_score on the device tensors t = (x, lig_r, lig_f, rec, rec_r, rec_f, pairs) into sentinel-filled outputs."""
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs = t
    S, n = x.shape[0], x.shape[1]
    e = torch.full((S, 7), sentinel, dtype=torch.float64, device=x.device)
    g = torch.full((S, n, 3), sentinel, dtype=torch.float64, device=x.device) if with_grad else None
    LA.pose_score(x, lig_r, lig_f, rec, rec_r, rec_f, CFG, DIV, pairs if with_pairs else None, energy=e, grad=g)
    return e, g


def _case(S, n, m, seed, per_sample=False, with_pairs=True):
    t, ref = as_torch(V.random_case(S, n, m, seed, per_sample, with_pairs))
    return [None if a is None else a.to(_dev()) for a in t], ref


# ---------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("n,m", [(1, 1), (4, 0), (37, 1023), (37, 1024), (37, 1025), (300, 2500), (1024, 64)])
def test_kernel_matches_the_fp64_restatement(n, m):
    for with_pairs in (True, False):
        t, ref = _case(3, n, m, 77 * n + m + with_pairs, with_pairs=with_pairs)
        e, g = _launch(t, with_pairs=with_pairs)
        check_against_ref(e.cpu().numpy(), g.cpu().numpy(), ref, f"n={n} m={m} pairs={with_pairs}")
        e2, none = _launch(t, with_grad=False, with_pairs=with_pairs)
        assert none is None and torch.equal(_bits(e), _bits(e2)), "energies with and without the gradient differ"
        if m == 0:
            assert torch.equal(e[:, :5], torch.zeros(3, 5, dtype=torch.float64, device=e.device)) and torch.equal(e[:, 6], e[:, 4])
        if not with_pairs:
            assert torch.equal(e[:, 5], torch.zeros(3, dtype=torch.float64, device=e.device))
    if n >= 37:
        assert bool((t[1] < 0).any()) and bool((t[4] < 0).any()) and (ref["energy"][:, :4] > 0).all()      # untyped atoms; every term
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. reproducibility
def test_two_launches_and_batch_positions_give_the_same_bits():
    t, _ = _case(5, 37, 1300, 5)
    e, g = _launch(t)
    e2, g2 = _launch(t)
    assert torch.equal(_bits(e), _bits(e2)) and torch.equal(_bits(g), _bits(g2)), "two launches differ"
    for s in range(5):
        one = [t[0][s:s + 1].contiguous()] + t[1:]
        e1, g1 = _launch(one)
        assert torch.equal(_bits(e1[0]), _bits(e[s])) and torch.equal(_bits(g1[0]), _bits(g[s])), s
    en, _ = _launch(t, with_grad=False)
    assert torch.equal(_bits(en), _bits(e))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3. receptor stride
def test_per_sample_receptors_are_read_through_the_stride():
    t, ref = _case(3, 37, 1100, 11, per_sample=True)
    e, g = _launch(t)
    check_against_ref(e.cpu().numpy(), g.cpu().numpy(), ref, "per-sample receptors")
    assert not torch.equal(e[0], e[1])
    # one receptor replicated for every sample: stride 3 m and stride 0 give the same bits
    shared = t[3][1].contiguous()
    rep = shared[None].repeat(3, 1, 1).contiguous()
    e_rep, g_rep = _launch(t[:3] + [rep] + t[4:])
    e_one, g_one = _launch(t[:3] + [shared] + t[4:])
    assert torch.equal(_bits(e_rep), _bits(e_one)) and torch.equal(_bits(g_rep), _bits(g_one))
    assert torch.equal(_bits(e_rep[1]), _bits(e[1]))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 4. limits and return codes
def test_limits_return_codes_and_empty_calls():
    dev = _dev()
    lib = L.load()
    t, _ = _case(2, 8, 5, 3)
    x, lig_r, lig_f, rec, rec_r, rec_f, pairs = t
    e = torch.full((2, 7), -7.0, dtype=torch.float64, device=dev)

    def args(**kw):
        a = L.ScoreArgs(n_samples=2, n=8, m=5, rec_stride=0, pos=x.data_ptr(), lig_radii=lig_r.data_ptr(), lig_flags=lig_f.data_ptr(),
                        rec=rec.data_ptr(), rec_radii=rec_r.data_ptr(), rec_flags=rec_f.data_ptr(), cutoff=8.0, gauss_offset=0.0,
                        gauss_width=0.8, hydrophobic_good=0.0, hydrophobic_bad=2.5, hbond_good=-0.6, hbond_bad=0.0, w_gauss=-0.045,
                        w_repulsion=0.8, w_hydrophobic=-0.035, w_hbond=-0.6, tor_divisor=1.0, energy=e.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rc(**kw):
        return lib.ddp_pose_score(ctypes.byref(args(**kw)), LA.stream())

    assert rc(n=L.DDP_EVAL_MAX_ATOMS + 1) == -2                                                       # DDP_ELIMIT
    for bad in (dict(pos=None), dict(lig_radii=None), dict(lig_flags=None), dict(energy=None), dict(rec=None), dict(rec_radii=None),
                dict(rec_flags=None), dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=float("inf")), dict(cutoff=float("nan")),
                dict(n_samples=-1), dict(n=0), dict(n=-3), dict(m=-1), dict(rec_stride=14), dict(gauss_width=0.0), dict(tor_divisor=0.0),
                dict(hbond_bad=-0.6)):
        assert rc(**bad) == -1, bad                                                                   # DDP_EINVAL
    assert lib.ddp_pose_score(None, LA.stream()) == -1
    with pytest.raises(L.DdpError, match="DDP_EVAL_MAX_ATOMS"):
        big = torch.zeros(1, L.DDP_EVAL_MAX_ATOMS + 1, 3, device=dev)
        LA.pose_score(big, torch.ones(big.shape[1], device=dev), torch.zeros(big.shape[1], dtype=torch.uint8, device=dev), rec, rec_r, rec_f, CFG)
    # nothing above launched, n_samples = 0 returns 0 and launches nothing: the sentinel-filled output is untouched
    assert rc(n_samples=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(e, torch.full((2, 7), -7.0, dtype=torch.float64, device=dev))
    assert LA.pose_score(x[:0], lig_r, lig_f, rec, rec_r, rec_f, CFG)[0].shape == (0, 7)
    # m = 0 needs no receptor pointers; a valid call does write
    assert rc(m=0, rec=None, rec_radii=None, rec_flags=None) == 0 and rc() == 0
    torch.cuda.synchronize()
    assert bool((e != -7.0).all())
    # shapes are checked on the host
    with pytest.raises(L.DdpError, match="self_pairs"):
        LA.pose_score(x, lig_r, lig_f, rec, rec_r, rec_f, CFG, self_pairs=torch.zeros(4, 4, dtype=torch.uint8, device=dev))
    with pytest.raises(L.DdpError, match="lig_flags"):
        LA.pose_score(x, lig_r, lig_f.to(torch.int32), rec, rec_r, rec_f, CFG)
    with pytest.raises(L.DdpError, match="rec"):
        LA.pose_score(x, lig_r, lig_f, rec[None].repeat(3, 1, 1), rec_r, rec_f, CFG)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 5. the scorer on the device
def _scorer_bound(cpu: SC.PoseScores, sc: SC.PoseScorer, x, atom_pos=None):
    """vinardo_ref on the scorer's own tables: (reference dict, bounds) for the poses x."""
    t = sc._cpu
    rec = t["rec"] if atom_pos is None else atom_pos
    return V.score(x.numpy(), t["lig_r"].numpy(), t["lig_f"].numpy(), rec.numpy(), t["rec_r"].numpy(), t["rec_f"].numpy(),
                   t["pairs"].numpy(), sc.tor_divisor)


def _check_scores(dev_scores, cpu_scores, ref):
    be, bg = V.bounds(ref)
    d, c = dev_scores.cpu(), cpu_scores
    for got in (d, c):                                   # both forms sit within the bound of the restatement ...
        e = torch.cat([got.terms, got.inter[:, None], got.intra[:, None], got.total[:, None]], 1).numpy()
        assert (np.abs(e - ref["energy"]) <= be).all()
        assert (np.abs(got.grad.numpy() - ref["grad"]) <= bg[:, None, None]).all()
    e_d = torch.cat([d.terms, d.inter[:, None], d.intra[:, None], d.total[:, None]], 1).numpy()
    e_c = torch.cat([c.terms, c.inter[:, None], c.intra[:, None], c.total[:, None]], 1).numpy()
    assert (np.abs(e_d - e_c) <= be).all() and (np.abs(d.grad.numpy() - c.grad.numpy()) <= bg[:, None, None]).all()   # ... and of each other


def test_device_scorer_matches_the_cpu_scorer_on_3dpf():
    dev = _dev()
    g, pdb, full = fixture_3dpf()
    x = perturbed_poses()
    for receptor in ("graph", full):
        cpu, gpu = SC.PoseScorer(g, receptor=receptor), SC.PoseScorer(g, dev, receptor=receptor)
        got = gpu.score(x.to(dev), with_grad=True)
        assert got.total.is_cuda and got.total.dtype == torch.float64 and got.grad.shape == (16, 37, 3)
        _check_scores(got, cpu.score(x, with_grad=True), _scorer_bound(None, cpu, x))
        assert torch.equal(_bits(gpu.score(x.to(dev)).total), _bits(got.total)) and gpu.score(x.to(dev)).grad is None
    with pytest.raises(ValueError):
        cpu.score(x.to(dev))                                  # a CPU scorer does not take device poses
    # the flexible graph with each sample's own atom positions
    gf, _ = graph_3dpf(flex="A:160-A:193-A:197")
    cpu, gpu = SC.PoseScorer(gf), SC.PoseScorer(gf, dev)
    gen = torch.Generator().manual_seed(4)
    apos = (gf["atom"].pos.float()[None] + 0.2 * torch.randn(16, cpu.n_a, 3, generator=gen)).contiguous()
    got = gpu.score(x.to(dev), atom_pos=apos.to(dev), with_grad=True)
    _check_scores(got, cpu.score(x, atom_pos=apos, with_grad=True), _scorer_bound(None, cpu, x, apos))
    assert not torch.equal(got.total[0], gpu.score(x.to(dev)).total[0])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 6. NaN containment
def test_a_nan_coordinate_poisons_its_own_sample_only_on_the_device():
    dev = _dev()
    g, _, full = fixture_3dpf()
    sc = SC.PoseScorer(g, dev, receptor=full)
    x = perturbed_poses()[:4].to(dev)
    clean = sc.score(x, with_grad=True)
    bad = x.clone()
    bad[2, 5, 1] = float("nan")
    got = sc.score(bad, with_grad=True)
    assert bool(torch.isnan(got.total[2])) and bool(torch.isnan(got.inter[2])) and bool(torch.isnan(got.terms[2, 0]))
    for s in (0, 1, 3):
        assert torch.equal(_bits(got.terms[s]), _bits(clean.terms[s])) and torch.equal(_bits(got.total[s]), _bits(clean.total[s]))
        assert torch.equal(_bits(got.intra[s]), _bits(clean.intra[s])) and torch.equal(_bits(got.grad[s]), _bits(clean.grad[s]))
    # a NaN in one sample's own receptor (flexible graph): the same containment
    gf, _ = graph_3dpf(flex="A:160-A:193-A:197")
    sf = SC.PoseScorer(gf, dev)
    apos = gf["atom"].pos.float()[None].repeat(4, 1, 1).contiguous().to(dev)
    ok = sf.score(x, atom_pos=apos)
    apos[1, 7, 0] = float("nan")
    got = sf.score(x, atom_pos=apos)
    assert bool(torch.isnan(got.total[1])) and all(torch.equal(_bits(got.total[s]), _bits(ok.total[s])) for s in (0, 2, 3))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7. the driver on the device
class DeviceStub:
    """The stub score model of test_inference_csv (a pure function of the batch positions, the same arithmetic) with every output
    created on the positions' device: the device sampler hands the outputs' addresses to its update kernels."""
    flexible_sidechains = True

    def __call__(self, b):
        B = b.num_graphs
        lp = b["ligand"].pos.reshape(B, -1, 3)
        c = lp.mean(1)
        tr = -0.05 * c
        rot = 0.02 * torch.stack([c[:, 1], -c[:, 0], c[:, 2]], 1)
        T = int(b["ligand"].edge_mask.sum())
        tor = 0.01 * lp[:, :1, 0].expand(B, T // B).reshape(-1) if T else torch.empty(0, device=lp.device)
        S = b["flexResidues"].edge_idx.shape[0] if len(b["flexResidues"]) > 0 else 0
        return tr.contiguous(), rot.contiguous(), tor.contiguous(), 0.01 * torch.ones(S, device=lp.device)


def test_run_csv_on_the_device_matches_the_cpu_run(tmp_path):
    """The stub model is a pure function of the positions and runs on either device; the sampler's arithmetic differs between the
    devices in the last fp32 bits of the poses, so each run's scores are checked against the restatement on ITS OWN poses within the
    bound, and the two runs' scores against each other within the bound plus what a pose difference of that size can move them:
    |dE| <= sum_i |grad_i| |dx_i| to first order, taken with twice the CPU scorer's own gradient of inter (the divisor only shrinks
    it) and the largest coordinate difference seen."""
    from test_inference_csv import StubConfidence
    dev = _dev()
    p = tmp_path / "complexes.csv"
    p.write_text(CSV)

    def run(device):
        return INF.run_csv(str(p), DeviceStub(), device, confidence_model=StubConfidence(), samples_per_complex=4, inference_steps=2,
                           root=GOLDEN, seed=2, allow_zero_esm=True, rank_by="score")

    on_cpu, on_dev = run(torch.device("cpu")), run(dev)
    g, pdb, full = fixture_3dpf()
    cpu_rigid = SC.PoseScorer(g, receptor=full)
    for k, (a, b) in enumerate(zip(on_cpu, on_dev)):
        assert a.skipped is None and b.skipped is None and not b.scores.total.is_cuda
        assert a.order.tolist() == b.order.tolist()
        dx = float((a.ligand_pos.double() - b.ligand_pos.double()).abs().max())
        assert dx < 1e-3
        if k == 1:          # the rigid row: the full PDB receptor, the same on both devices
            for r in (a, b):
                ref = _scorer_bound(None, cpu_rigid, r.ligand_pos)
                be, _ = V.bounds(ref)
                assert (np.abs(r.scores.total.numpy() - ref["energy"][:, 6]) <= be[:, 6]).all()
                assert (np.abs(r.scores.terms.numpy() - ref["energy"][:, :4]) <= be[:, :4]).all()
            # the device run's scores are the CPU scorer's scores of the same poses, within the bound
            same = cpu_rigid.score(b.ligand_pos)
            assert (np.abs(b.scores.total.numpy() - same.total.numpy()) <= be[:, 6]).all()
            assert (np.abs(b.scores.terms.numpy() - same.terms.numpy()) <= be[:, :4]).all()
            slack = 2.0 * dx * cpu_rigid.score(a.ligand_pos, with_grad=True).grad.abs().sum((1, 2)).numpy()
            assert (np.abs(a.scores.total.numpy() - b.scores.total.numpy()) <= be[:, 6] + slack).all()
    torch.cuda.synchronize()
